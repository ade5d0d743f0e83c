// raster_geometry.hip -- geometry terms of the mesh deformer (C-ABI and the DEFINITIONS: include/gd_mesh_geometry.h):
// face / vertex normals of a moving mesh, the uniform Laplacian loss and the normal-consistency loss, forward and backward
// (Garment_Deformer_NeTF/deformer/core/mesh.py:82-94, losses/laplacian.py, losses/normal_consistency.py).  Built with
// -ffp-contract=off: the header fixes the order of every operation.
//
// These are latency- and bandwidth-trivial at the deformer's sizes (tens of thousands of vertices): one thread per
// element, plain loads, nothing tuned.  What the file is for is the contract of raster_mesh.hip: no floating-point atomics
// anywhere, so reruns are bit-identical.
//   normals forward    face_normals (thread per face) -> vertex_normals (thread per vertex, gathers its corners in CSR order)
//   normals backward   normals_corner_grad (thread per face, [F][3][4] slab) -> corner_sum3 (thread per vertex, CSR order):
//                      the corner_grad + vertex_sum shape of raster_mesh.hip.  vertex_sum_kernel itself is not shared: it
//                      writes as many components per vertex as the slab holds per corner, [V][4] for a float4 slab, and
//                      dverts is [V][3].
//   scatter-free sums  a loss is reduced per workgroup in a fixed LDS tree into partials, then by one workgroup.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gd_mesh_geometry.h"
#include "raster_mesh_common.h"

namespace gd {
namespace {

constexpr float kCosEps = 1e-8f;     // torch.cosine_similarity

// adjoint of n = x / max(l, eps), l = |x|
__device__ __forceinline__ V3 normalize_adjoint(V3 n, float l, V3 g)
{
    if (l > kNormEps) return divide(sub(g, scale(n, dot(n, g))), l);
    return divide(g, kNormEps);
}

__device__ __forceinline__ bool face_corners(const int* __restrict__ tri, int f, int V, int idx[3])
{
    idx[0] = tri[3 * (size_t)f];
    idx[1] = tri[3 * (size_t)f + 1];
    idx[2] = tri[3 * (size_t)f + 2];
    return (unsigned)idx[0] < (unsigned)V && (unsigned)idx[1] < (unsigned)V && (unsigned)idx[2] < (unsigned)V;
}

// ---- normals ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void face_normals_kernel(int V, int F, const float* __restrict__ verts,
                                                           const int* __restrict__ tri, float* __restrict__ fn)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int idx[3];
    V3 n = V3{0.0f, 0.0f, 0.0f};
    if (face_corners(tri, f, V, idx)) {
        const V3 a = load3(verts, idx[0]);
        const V3 c = cross(sub(load3(verts, idx[1]), a), sub(load3(verts, idx[2]), a));
        n = divide(c, fmaxf(norm(c), kNormEps));
    }
    store3(fn, f, n);
}

__global__ __launch_bounds__(256) void vertex_normals_kernel(int V, int F, const int* __restrict__ corner_ptr,
                                                             const int* __restrict__ corner_idx,
                                                             const float* __restrict__ fn, float* __restrict__ vn,
                                                             float* __restrict__ len)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int a = max(corner_ptr[v], 0), b = min(corner_ptr[v + 1], 3 * F);
    V3 s = V3{0.0f, 0.0f, 0.0f};
    for (int j = a; j < b; j++) {
        const int corner = corner_idx[j];
        if ((unsigned)corner < (unsigned)(3 * F)) s = add(s, load3(fn, corner / 3));
    }
    const float l = norm(s);
    len[v] = l;
    store3(vn, v, divide(s, fmaxf(l, kNormEps)));
}

__global__ __launch_bounds__(256) void normals_corner_grad_kernel(int V, int F, const float* __restrict__ verts,
                                                                  const int* __restrict__ tri,
                                                                  const float* __restrict__ vn,
                                                                  const float* __restrict__ len,
                                                                  const float* __restrict__ dvn,
                                                                  const float* __restrict__ dfn,
                                                                  float4* __restrict__ slab)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int idx[3];
    V3 g[3] = {V3{0.0f, 0.0f, 0.0f}, V3{0.0f, 0.0f, 0.0f}, V3{0.0f, 0.0f, 0.0f}};
    if (face_corners(tri, f, V, idx)) {
        const V3 a = load3(verts, idx[0]);
        const V3 u = sub(load3(verts, idx[1]), a), w = sub(load3(verts, idx[2]), a);
        const V3 c = cross(u, w);
        const float lc = norm(c);
        const V3 n = divide(c, fmaxf(lc, kNormEps));
        V3 G = dfn ? load3(dfn, f) : V3{0.0f, 0.0f, 0.0f};
        if (dvn) {
#pragma unroll
            for (int i = 0; i < 3; i++)
                G = add(G, normalize_adjoint(load3(vn, idx[i]), len[idx[i]], load3(dvn, idx[i])));
        }
        const V3 Gc = normalize_adjoint(n, lc, G);
        const V3 du = cross(w, Gc), dw = cross(Gc, u);
        g[0] = sub(V3{-du.x, -du.y, -du.z}, dw);
        g[1] = du;
        g[2] = dw;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) slab[(size_t)f * 3 + i] = make_float4(g[i].x, g[i].y, g[i].z, 0.0f);
}

__global__ __launch_bounds__(256) void corner_sum3_kernel(int V, int F, const int* __restrict__ corner_ptr,
                                                          const int* __restrict__ corner_idx,
                                                          const float4* __restrict__ slab, float* __restrict__ dverts)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int a = max(corner_ptr[v], 0), b = min(corner_ptr[v + 1], 3 * F);
    V3 s = V3{0.0f, 0.0f, 0.0f};
    for (int j = a; j < b; j++) {
        const int corner = corner_idx[j];
        if ((unsigned)corner < (unsigned)(3 * F)) {
            const float4 r = slab[corner];
            s = add(s, V3{r.x, r.y, r.z});
        }
    }
    store3(dverts, v, s);
}

// ---- the fixed-order sum -----------------------------------------------------------------------------------------------

// loss = (sum of n partials) / denom, or 0 if denom <= 0
__global__ __launch_bounds__(256) void reduce_partials_kernel(int n, const float* __restrict__ partials, int denom,
                                                              float* __restrict__ loss)
{
    __shared__ float lds[256];
    float x = 0.0f;
    for (int i = threadIdx.x; i < n; i += 256) x += partials[i];
    const float total = block_tree_sum(x, lds);
    if (threadIdx.x == 0) *loss = denom > 0 ? total / (float)denom : 0.0f;
}

// ---- uniform Laplacian ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void laplacian_forward_kernel(int V, int N, const float* __restrict__ verts,
                                                                const int* __restrict__ nbr_ptr,
                                                                const int* __restrict__ nbr_idx,
                                                                float* __restrict__ delta, float* __restrict__ partials)
{
    __shared__ float lds[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float sq = 0.0f;
    if (i < V) {
        const int a = max(nbr_ptr[i], 0), b = min(nbr_ptr[i + 1], N);
        const int deg = nbr_ptr[i + 1] - nbr_ptr[i];
        const V3 v = load3(verts, i);
        V3 s = V3{0.0f, 0.0f, 0.0f};
        for (int j = a; j < b; j++) {
            const int k = nbr_idx[j];
            if ((unsigned)k < (unsigned)V) s = add(s, load3(verts, k));
        }
        const V3 d = deg > 0 ? sub(divide(s, (float)deg), v) : V3{-v.x, -v.y, -v.z};
        store3(delta, i, d);
        sq = dot(d, d);
    }
    const float total = block_tree_sum(sq, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void laplacian_backward_kernel(int V, int N, const int* __restrict__ nbr_ptr,
                                                                 const int* __restrict__ nbr_idx,
                                                                 const float* __restrict__ delta,
                                                                 const float* __restrict__ dloss,
                                                                 float* __restrict__ dverts)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= V) return;
    const int a = max(nbr_ptr[k], 0), b = min(nbr_ptr[k + 1], N);
    V3 s = V3{0.0f, 0.0f, 0.0f};
    for (int j = a; j < b; j++) {
        const int n = nbr_idx[j];
        if ((unsigned)n >= (unsigned)V) continue;
        const int deg = nbr_ptr[n + 1] - nbr_ptr[n];
        if (deg > 0) s = add(s, divide(load3(delta, n), (float)deg));
    }
    const float w = *dloss * (2.0f / (float)V);
    store3(dverts, k, scale(sub(s, load3(delta, k)), w));
}

// ---- normal consistency --------------------------------------------------------------------------------------------------

__device__ __forceinline__ float clamped_norm(V3 a) { return fmaxf(norm(a), kCosEps); }

__global__ __launch_bounds__(256) void consistency_forward_kernel(int F, const float* __restrict__ fn,
                                                                  const int* __restrict__ face_nbr,
                                                                  float* __restrict__ partials)
{
    __shared__ float lds[256];
    const int f = blockIdx.x * 256 + threadIdx.x;
    float sum = 0.0f;
    if (f < F) {
        const V3 nf = load3(fn, f);
        const float mf = clamped_norm(nf);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int g = face_nbr[3 * (size_t)f + i];
            if (g <= f || g >= F) continue;
            const V3 ng = load3(fn, g);
            const float c = dot(nf, ng) / (mf * clamped_norm(ng));
            sum += (1.0f - c) * (1.0f - c);
        }
    }
    const float total = block_tree_sum(sum, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void consistency_backward_kernel(int F, int P, const float* __restrict__ fn,
                                                                   const int* __restrict__ face_nbr,
                                                                   const float* __restrict__ dloss,
                                                                   float* __restrict__ dfn)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    V3 s = V3{0.0f, 0.0f, 0.0f};
    if (P > 0) {
        const V3 nf = load3(fn, f);
        const float lf = norm(nf), mf = fmaxf(lf, kCosEps);
        const float w = *dloss / (float)P;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int g = face_nbr[3 * (size_t)f + i];
            if (g < 0 || g >= F || g == f) continue;
            const V3 ng = load3(fn, g);
            const float mg = clamped_norm(ng);
            const float c = dot(nf, ng) / (mf * mg);
            V3 D = divide(ng, mg);
            if (lf > kCosEps) D = sub(D, divide(scale(nf, c), mf));
            D = divide(D, mf);
            s = add(s, scale(D, w * (-2.0f * (1.0f - c))));
        }
    }
    store3(dfn, f, s);
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace
}  // namespace gd

extern "C" {

int gd_mesh_normals_forward(void* stream, int V, int F, const float* verts, const int* tri, const int* corner_ptr,
                            const int* corner_idx, float* fn, float* vn, float* len)
{
    using namespace gd;
    if (V <= 0 || F < 0) return mesh_fail(-1, "normals: V must be positive and F >= 0");
    if (F >= (1 << 29)) return mesh_fail(-1, "normals: F must be < 2^29");
    if (!verts || !corner_ptr || !vn || !len || (F > 0 && (!tri || !corner_idx || !fn)))
        return mesh_fail(-1, "normals: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (F > 0) hipLaunchKernelGGL(face_normals_kernel, grid_of(F), dim3(256), 0, s, V, F, verts, tri, fn);
    hipLaunchKernelGGL(vertex_normals_kernel, grid_of(V), dim3(256), 0, s, V, F, corner_ptr, corner_idx, fn, vn, len);
    return mesh_launched(nullptr, "normals forward");
}

size_t gd_mesh_normals_backward_scratch_bytes(int F)
{
    if (F < 0) return 0;
    return gd::align256((size_t)F * 3 * 4 * sizeof(float));
}

int gd_mesh_normals_backward(void* stream, int V, int F, const float* verts, const int* tri, const int* corner_ptr,
                             const int* corner_idx, const float* vn, const float* len, const float* dvn,
                             const float* dfn, float* dverts, void* scratch)
{
    using namespace gd;
    if (V <= 0 || F < 0) return mesh_fail(-1, "normals backward: V must be positive and F >= 0");
    if (F >= (1 << 29)) return mesh_fail(-1, "normals backward: F must be < 2^29");
    if (!verts || !corner_ptr || !dverts || (dvn && (!vn || !len)) || (F > 0 && (!tri || !corner_idx || !scratch)))
        return mesh_fail(-1, "normals backward: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (F > 0)
        hipLaunchKernelGGL(normals_corner_grad_kernel, grid_of(F), dim3(256), 0, s, V, F, verts, tri, vn, len, dvn, dfn,
                           (float4*)scratch);
    hipLaunchKernelGGL(corner_sum3_kernel, grid_of(V), dim3(256), 0, s, V, F, corner_ptr, corner_idx,
                       (const float4*)scratch, dverts);
    return mesh_launched(nullptr, "normals backward");
}

size_t gd_mesh_loss_scratch_bytes(int n)
{
    if (n < 0) return 0;
    return gd::align256(((size_t)n + 255) / 256 * sizeof(float));
}

int gd_mesh_laplacian_forward(void* stream, int V, int N, const float* verts, const int* nbr_ptr, const int* nbr_idx,
                              float* delta, float* loss, void* scratch)
{
    using namespace gd;
    if (V <= 0 || N < 0) return mesh_fail(-1, "laplacian: V must be positive and N >= 0");
    if (!verts || !nbr_ptr || !delta || !loss || !scratch || (N > 0 && !nbr_idx))
        return mesh_fail(-1, "laplacian: null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(laplacian_forward_kernel, grid_of(V), dim3(256), 0, s, V, N, verts, nbr_ptr, nbr_idx, delta,
                       (float*)scratch);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, s, (V + 255) / 256, (const float*)scratch, V, loss);
    return mesh_launched(nullptr, "laplacian forward");
}

int gd_mesh_laplacian_backward(void* stream, int V, int N, const int* nbr_ptr, const int* nbr_idx, const float* delta,
                               const float* dloss, float* dverts)
{
    using namespace gd;
    if (V <= 0 || N < 0) return mesh_fail(-1, "laplacian backward: V must be positive and N >= 0");
    if (!nbr_ptr || !delta || !dloss || !dverts || (N > 0 && !nbr_idx))
        return mesh_fail(-1, "laplacian backward: null pointer");
    hipLaunchKernelGGL(laplacian_backward_kernel, grid_of(V), dim3(256), 0, (hipStream_t)stream, V, N, nbr_ptr, nbr_idx,
                       delta, dloss, dverts);
    return mesh_launched(nullptr, "laplacian backward");
}

int gd_mesh_normal_consistency_forward(void* stream, int F, int P, const float* fn, const int* face_nbr, float* loss,
                                       void* scratch)
{
    using namespace gd;
    if (F < 0 || P < 0) return mesh_fail(-1, "normal consistency: F and P must be >= 0");
    if (!loss || !scratch || (F > 0 && (!fn || !face_nbr))) return mesh_fail(-1, "normal consistency: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (F > 0)
        hipLaunchKernelGGL(consistency_forward_kernel, grid_of(F), dim3(256), 0, s, F, fn, face_nbr, (float*)scratch);
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(256), 0, s, (F + 255) / 256, (const float*)scratch, P, loss);
    return mesh_launched(nullptr, "normal consistency forward");
}

int gd_mesh_normal_consistency_backward(void* stream, int F, int P, const float* fn, const int* face_nbr,
                                        const float* dloss, float* dfn)
{
    using namespace gd;
    if (F < 0 || P < 0) return mesh_fail(-1, "normal consistency backward: F and P must be >= 0");
    if (F == 0) return 0;
    if (!fn || !face_nbr || !dloss || !dfn) return mesh_fail(-1, "normal consistency backward: null pointer");
    hipLaunchKernelGGL(consistency_backward_kernel, grid_of(F), dim3(256), 0, (hipStream_t)stream, F, P, fn, face_nbr,
                       dloss, dfn);
    return mesh_launched(nullptr, "normal consistency backward");
}

}  // extern "C"
