// raster_mesh_common.h -- device and host primitives shared by the mesh translation units of libgd_raster.so
// (raster_geometry, raster_remesh, raster_simplify, raster_atlas, raster_clean, raster_shader, raster_gbuffer_losses): the
// three-component vector math, the range check, the order keys of exact bounds, the root walk of the hooking forests, the
// fixed LDS tree sum, the connectivity tables of include/gd_mesh_remesh.h with the collapse tests and
// ring walks that stand on them, and the camera terms of the two shading files.  Internal to garmentdreamer_amd/csrc.
// One definition each: these files are built with -ffp-contract=off and compared bit for bit with numpy statements, and
// the ORDER of every operation below (the parentheses of dot, the strides of block_tree_sum) is fixed by
// include/gd_mesh_*.h -- a second copy is a second place for that contract to drift.  Everything on the device side is
// __forceinline__ and the library is built without relocatable device code: each translation unit keeps its own copy
// under its own compile flags, and moving a helper here does not change the instructions of a kernel that uses it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gd_mesh_remesh.h"
#include "raster_common.h"

namespace gd {

typedef unsigned long long u64;       // the type of HIP's 64-bit atomicMin
constexpr float kNormEps = 1e-12f;    // torch.nn.functional.normalize

// ---- vectors --------------------------------------------------------------------------------------------------------
template <typename T>
struct Vec3 {
    T x, y, z;
};
using V3 = Vec3<float>;
using D3 = Vec3<double>;

// vertex tables are fp32; load3<double> converts on the way in
template <typename T = float>
__device__ __forceinline__ Vec3<T> load3(const float* __restrict__ p, size_t i)
{
    return Vec3<T>{(T)p[3 * i], (T)p[3 * i + 1], (T)p[3 * i + 2]};
}
__device__ __forceinline__ void store3(float* __restrict__ p, size_t i, V3 v)
{
    p[3 * i] = v.x;
    p[3 * i + 1] = v.y;
    p[3 * i + 2] = v.z;
}
template <typename T>
__device__ __forceinline__ Vec3<T> add(Vec3<T> a, Vec3<T> b) { return Vec3<T>{a.x + b.x, a.y + b.y, a.z + b.z}; }
template <typename T>
__device__ __forceinline__ Vec3<T> sub(Vec3<T> a, Vec3<T> b) { return Vec3<T>{a.x - b.x, a.y - b.y, a.z - b.z}; }
template <typename T>
__device__ __forceinline__ Vec3<T> scale(Vec3<T> a, T s) { return Vec3<T>{a.x * s, a.y * s, a.z * s}; }
template <typename T>
__device__ __forceinline__ Vec3<T> divide(Vec3<T> a, T s) { return Vec3<T>{a.x / s, a.y / s, a.z / s}; }
template <typename T>
__device__ __forceinline__ T dot(Vec3<T> a, Vec3<T> b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ float norm(V3 a) { return sqrtf(dot(a, a)); }
template <typename T>
__device__ __forceinline__ Vec3<T> cross(Vec3<T> u, Vec3<T> w)
{
    return Vec3<T>{u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
}
template <typename T>
__device__ __forceinline__ Vec3<T> tri_normal(Vec3<T> p0, Vec3<T> p1, Vec3<T> p2)
{
    return cross(sub(p1, p0), sub(p2, p0));
}
template <typename T>
__device__ __forceinline__ T sqlen(Vec3<T> a, Vec3<T> b)
{
    const Vec3<T> d = sub(a, b);
    return dot(d, d);
}
template <typename T>
__device__ __forceinline__ Vec3<T> midpoint(Vec3<T> a, Vec3<T> b)
{
    return Vec3<T>{0.5f * (a.x + b.x), 0.5f * (a.y + b.y), 0.5f * (a.z + b.z)};
}

// ---- range check and the fixed-order sum ----------------------------------------------------------------------------
__device__ __forceinline__ bool in_range(int i, int n) { return (unsigned)i < (unsigned)n; }

// The order-preserving integer key of a float (include/gd_atlas.h section 3): finite floats compare as the reals do, -0 below
// +0, so an exact minimum or maximum can be taken by integer atomics; order_value is its inverse.
__device__ __forceinline__ uint32_t order_key(float x)
{
    const uint32_t u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float order_value(uint32_t k)
{
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// The root of x in a hooking forest with parent[y] <= y (include/gd_atlas.h section 2), so the walk ends.  Relaxed
// device-scope loads: other workgroups lower parent while this walk runs.
__device__ __forceinline__ int root_of(const int32_t* parent, int x, int n)
{
    int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x && in_range(p, n)) {
        x = p;
        p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return x;
}

// The headers' tree over the 256 values of a 256-thread workgroup (strides 128, 64, ... 1); every thread receives the total.
template <typename T>
__device__ __forceinline__ T block_tree_sum(T x, T* lds)
{
    const int t = threadIdx.x;
    lds[t] = x;
    __syncthreads();
#pragma unroll
    for (int stride = 128; stride > 0; stride >>= 1) {
        if (t < stride) lds[t] += lds[t + stride];
        __syncthreads();
    }
    return lds[0];
}

// ---- mesh tables (gd_remesh_mesh of include/gd_mesh_remesh.h, by value as a kernel argument) ------------------------
struct Conn {
    int V, F, E;
    const float* verts;
    const int *tri, *ev, *eh, *bnd, *nbr_ptr, *nbr_idx, *vf_ptr, *vf_idx;
};

constexpr int kMaxFaces = 1 << 29;   // 3F and every corner index stay below 2^31

inline Conn conn_of(const gd_remesh_mesh* m)
{
    return Conn{m->V, m->F, m->E, m->verts, m->tri, m->ev, m->eh, m->bnd, m->nbr_ptr, m->nbr_idx, m->vf_ptr, m->vf_idx};
}

// nonempty: the simplifier's entries need at least one face and one edge; the remesher's admit an empty mesh
inline bool mesh_ok(const gd_remesh_mesh* m, bool nonempty)
{
    const int least = nonempty ? 1 : 0;
    return m && m->V > 0 && m->F >= least && m->F < kMaxFaces && m->E >= least && m->E <= 3 * m->F && m->verts && m->tri &&
           m->ev && m->eh && m->bnd && m->nbr_ptr && m->nbr_idx && m->vf_ptr && m->vf_idx;
}

// one lane per element, 256 per workgroup
inline dim3 grid_of(int n) { return dim3((unsigned)((max(n, 1) + 255) / 256)); }

// ---- collapse tests -------------------------------------------------------------------------------------------------
// The number of common neighbours of a and b (a merge walk over their two ascending rows); the first two go to `opposite`.
__device__ __forceinline__ int common_neighbours(const Conn& m, int a, int b, int opposite[2])
{
    const int a0 = m.nbr_ptr[a], a1 = m.nbr_ptr[a + 1], b0 = m.nbr_ptr[b], b1 = m.nbr_ptr[b + 1];
    int common = 0;
    for (int i = a0, j = b0; i < a1 && j < b1;) {
        const int x = m.nbr_idx[i], y = m.nbr_idx[j];
        if (x == y) {
            if (common < 2) opposite[common] = x;
            common++;
            i++;
            j++;
        } else if (x < y) i++;
        else j++;
    }
    return common;
}

// Does every face of a that survives the collapse a -> b keep the side its normal points to?  T: the precision of the test.
template <typename T>
__device__ __forceinline__ bool collapse_keeps_normals(const Conn& m, int a, int b)
{
    const Vec3<T> pb = load3<T>(m.verts, b);
    for (int j = m.vf_ptr[a]; j < m.vf_ptr[a + 1]; j++) {
        const int corner = m.vf_idx[j];
        if (!in_range(corner, 3 * m.F)) return false;
        const int f = corner / 3, i = corner - 3 * f;
        const int x0 = m.tri[3 * (size_t)f], x1 = m.tri[3 * (size_t)f + 1], x2 = m.tri[3 * (size_t)f + 2];
        if (x0 == b || x1 == b || x2 == b) continue;   // the face goes with the edge
        if (!in_range(x0, m.V) || !in_range(x1, m.V) || !in_range(x2, m.V)) return false;
        const Vec3<T> p0 = load3<T>(m.verts, x0), p1 = load3<T>(m.verts, x1), p2 = load3<T>(m.verts, x2);
        const Vec3<T> before = tri_normal(p0, p1, p2);
        // selects: no indexed array
        const Vec3<T> after = tri_normal(i == 0 ? pb : p0, i == 1 ? pb : p1, i == 2 ? pb : p2);
        if (!(dot(before, after) > (T)0)) return false;
    }
    return true;
}

// ---- the ring of an edge --------------------------------------------------------------------------------------------
// f(v) for lo, for hi, then for every in-range neighbour of lo and of hi, in that order; stops and returns false as soon
// as f does.  A lambda captures its pointers BY VALUE: captured by reference, a __restrict__ kernel argument is reloaded
// through the closure and the walk is no longer the loop the compiler made of the spelled-out form.
template <typename Fn>
__device__ __forceinline__ bool for_each_ring_vertex(const Conn& m, int lo, int hi, Fn f)
{
    if (!f(lo) || !f(hi)) return false;
    for (int s = 0; s < 2; s++) {
        const int v = s ? hi : lo;
        for (int i = m.nbr_ptr[v]; i < m.nbr_ptr[v + 1]; i++) {
            const int n = m.nbr_idx[i];
            if (in_range(n, m.V) && !f(n)) return false;
        }
    }
    return true;
}

// the minimum of key onto lo, hi and both their neighbourhoods
__device__ __forceinline__ void spread_key(const Conn& m, int lo, int hi, u64 key, u64* __restrict__ vkey)
{
    for_each_ring_vertex(m, lo, hi, [vkey, key](int v) {
        atomicMin(&vkey[v], key);
        return true;
    });
}

// did key win on all of them?
__device__ __forceinline__ bool holds_key(const Conn& m, int lo, int hi, u64 key, const u64* __restrict__ vkey)
{
    return for_each_ring_vertex(m, lo, hi, [vkey, key](int v) { return vkey[v] == key; });
}

// ---- camera terms of the shading files (include/gd_shader.h, include/gd_mesh_losses.h) ------------------------------
// camera: [4][3] floats, the rows of R and the centre
struct Camera {
    V3 row[3];
    V3 center;
};

__device__ __forceinline__ Camera load_camera(const float* __restrict__ c)
{
    return Camera{{load3(c, 0), load3(c, 1), load3(c, 2)}, load3(c, 3)};
}

// n_cam = Rf (R n)
__device__ __forceinline__ V3 to_camera(const Camera& c, V3 n)
{
    return V3{dot(c.row[0], n), -dot(c.row[1], n), -dot(c.row[2], n)};
}

// u = (center - p) / max(l, 1e-12), l = |center - p|
__device__ __forceinline__ V3 unit_to_center(V3 center, V3 p, float* l)
{
    const V3 v = sub(center, p);
    *l = norm(v);
    return divide(v, fmaxf(*l, kNormEps));
}

// d = -Rf (R u)
__device__ __forceinline__ V3 view_direction(const Camera& c, V3 p, V3* u, float* l)
{
    *u = unit_to_center(c.center, p, l);
    return V3{-dot(c.row[0], *u), dot(c.row[1], *u), dot(c.row[2], *u)};
}

__device__ __forceinline__ float cosine(V3 a, V3 b, float eps)
{
    return dot(a, b) / (fmaxf(norm(a), eps) * fmaxf(norm(b), eps));
}

}  // namespace gd
