// raster_simplify.hip -- the deformer's final-mesh post-process on the device (C-ABI and the DEFINITIONS:
// include/gd_mesh_simplify.h): quadric-error decimation by half-edge collapses in rounds of independent sets, Taubin
// smoothing, and the rotation of the final mesh.  Built with -ffp-contract=off: the header fixes the order of every
// floating-point operation.  Quadrics, costs and the flip test are fp64; smoothing is fp32.
//
// Shape of every kernel, as in raster_remesh.hip: one lane per edge or vertex, loops only over CSR ranges, passes separated
// by kernel boundaries.  The only atomics are atomicMin on 64-bit keys and atomicAdd on one counter.  Every index read from
// a table is checked against its range before it is used to read or write.
//
// This runs once per deformation; nothing here is tuned.  The candidate kernel is bound by the divergence of its CSR rows
// and the spread kernel by scattered 8-byte atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_mesh_simplify.h"
#include "raster_common.h"

namespace gd {
namespace {

typedef unsigned long long u64;
constexpr int64_t kNoKey = INT64_MAX;

struct Conn {
    int V, F, E;
    const float* verts;
    const int *tri, *ev, *eh, *bnd, *nbr_ptr, *nbr_idx, *vf_ptr, *vf_idx;
};

struct D3 {
    double x, y, z;
};
__device__ __forceinline__ D3 loadd(const float* __restrict__ p, size_t i)
{
    return D3{(double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]};
}
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 u, D3 w)
{
    return D3{u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
}
__device__ __forceinline__ D3 tri_normal(D3 p0, D3 p1, D3 p2) { return cross(sub(p1, p0), sub(p2, p0)); }

__device__ __forceinline__ bool in_range(int i, int n) { return (unsigned)i < (unsigned)n; }

// ---- quadrics -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void quadrics_kernel(Conn m, double* __restrict__ Q)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= m.V) return;
    double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = m.vf_ptr[v]; j < m.vf_ptr[v + 1]; j++) {
        const int corner = m.vf_idx[j];
        if (!in_range(corner, 3 * m.F)) continue;
        const int f = corner / 3;
        const int x0 = m.tri[3 * (size_t)f], x1 = m.tri[3 * (size_t)f + 1], x2 = m.tri[3 * (size_t)f + 2];
        if (!in_range(x0, m.V) || !in_range(x1, m.V) || !in_range(x2, m.V)) continue;
        const D3 p0 = loadd(m.verts, x0);
        const D3 n = tri_normal(p0, loadd(m.verts, x1), loadd(m.verts, x2));
        const double d = -dot(n, p0);
        q[0] = q[0] + n.x * n.x;
        q[1] = q[1] + n.x * n.y;
        q[2] = q[2] + n.x * n.z;
        q[3] = q[3] + n.x * d;
        q[4] = q[4] + n.y * n.y;
        q[5] = q[5] + n.y * n.z;
        q[6] = q[6] + n.y * d;
        q[7] = q[7] + n.z * n.z;
        q[8] = q[8] + n.z * d;
        q[9] = q[9] + d * d;
    }
#pragma unroll
    for (int i = 0; i < 10; i++) Q[10 * (size_t)v + i] = q[i];
}

// ---- candidates ---------------------------------------------------------------------------------------------------------

// (Q[a] + Q[b])(p_b), clamped at +0
__device__ double collapse_cost(const Conn& m, const double* __restrict__ Q, int a, int b)
{
    double q[10];
#pragma unroll
    for (int i = 0; i < 10; i++) q[i] = Q[10 * (size_t)a + i] + Q[10 * (size_t)b + i];
    const D3 p = loadd(m.verts, b);
    const double squares = ((q[0] * p.x) * p.x + (q[4] * p.y) * p.y) + (q[7] * p.z) * p.z;
    const double mixed = ((q[1] * p.x) * p.y + (q[2] * p.x) * p.z) + (q[5] * p.y) * p.z;
    const double linear = (q[3] * p.x + q[6] * p.y) + q[8] * p.z;
    const double value = ((squares + 2.0 * mixed) + 2.0 * linear) + q[9];
    return value > 0.0 ? value : 0.0;
}

__device__ bool collapse_allowed(const Conn& m, int a, int b)
{
    if (m.bnd[a]) return false;
    const int a0 = m.nbr_ptr[a], a1 = m.nbr_ptr[a + 1], b0 = m.nbr_ptr[b], b1 = m.nbr_ptr[b + 1];
    int common = 0, opposite[2] = {-1, -1};
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
    if (common != 2) return false;
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int n = opposite[s];
        if (!in_range(n, m.V)) return false;
        if (!(m.nbr_ptr[n + 1] - m.nbr_ptr[n] > (m.bnd[n] ? 2 : 3))) return false;
    }
    const D3 pb = loadd(m.verts, b);
    for (int j = m.vf_ptr[a]; j < m.vf_ptr[a + 1]; j++) {
        const int corner = m.vf_idx[j];
        if (!in_range(corner, 3 * m.F)) return false;
        const int f = corner / 3, i = corner - 3 * f;
        const int x0 = m.tri[3 * (size_t)f], x1 = m.tri[3 * (size_t)f + 1], x2 = m.tri[3 * (size_t)f + 2];
        if (x0 == b || x1 == b || x2 == b) continue;   // the face goes with the edge
        if (!in_range(x0, m.V) || !in_range(x1, m.V) || !in_range(x2, m.V)) return false;
        const D3 p0 = loadd(m.verts, x0), p1 = loadd(m.verts, x1), p2 = loadd(m.verts, x2);
        const D3 before = tri_normal(p0, p1, p2);
        const D3 after = tri_normal(i == 0 ? pb : p0, i == 1 ? pb : p1, i == 2 ? pb : p2);   // selects: no indexed array
        if (!(dot(before, after) > 0.0)) return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void candidates_kernel(Conn m, const double* __restrict__ Q, int64_t* __restrict__ key,
                                                         int* __restrict__ dir, double* __restrict__ cost)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m.E) return;
    const int lo = m.ev[2 * (size_t)e], hi = m.ev[2 * (size_t)e + 1];
    int d = 0;
    int64_t k = kNoKey;
    double c[2] = {0.0, 0.0};
    if (in_range(lo, m.V) && in_range(hi, m.V) && lo != hi) {
        c[0] = collapse_cost(m, Q, lo, hi);
        c[1] = collapse_cost(m, Q, hi, lo);
        if (m.eh[2 * (size_t)e + 1] >= 0) {
            const int first = c[0] <= c[1] ? 1 : 2, second = 3 - first;
            if (collapse_allowed(m, first == 1 ? lo : hi, first == 1 ? hi : lo)) d = first;
            else if (collapse_allowed(m, second == 1 ? lo : hi, second == 1 ? hi : lo)) d = second;
            if (d) k = ((int64_t)__float_as_uint((float)(d == 1 ? c[0] : c[1])) << 32) | (int64_t)e;
        }
    }
    key[e] = k;
    dir[e] = d;
    cost[2 * (size_t)e] = c[0];
    cost[2 * (size_t)e + 1] = c[1];
}

// ---- passes -------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool is_live(int64_t k, int64_t threshold) { return k != kNoKey && k <= threshold; }

__global__ __launch_bounds__(256) void spread_kernel(Conn m, const int64_t* __restrict__ key,
                                                     const int64_t* __restrict__ threshold, const int* __restrict__ lock,
                                                     u64* __restrict__ vkey)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m.E) return;
    const int64_t k = key[e];
    if (!is_live(k, *threshold)) return;
    const int lo = m.ev[2 * (size_t)e], hi = m.ev[2 * (size_t)e + 1];
    if (!in_range(lo, m.V) || !in_range(hi, m.V)) return;
    if (lock[lo] || lock[hi]) return;
    for (int s = 0; s < 2; s++) {
        const int v = s ? hi : lo;
        for (int i = m.nbr_ptr[v]; i < m.nbr_ptr[v + 1]; i++) {
            const int n = m.nbr_idx[i];
            if (in_range(n, m.V) && lock[n]) return;
        }
    }
    atomicMin(&vkey[lo], (u64)k);
    atomicMin(&vkey[hi], (u64)k);
    for (int s = 0; s < 2; s++) {
        const int v = s ? hi : lo;
        for (int i = m.nbr_ptr[v]; i < m.nbr_ptr[v + 1]; i++) {
            const int n = m.nbr_idx[i];
            if (in_range(n, m.V)) atomicMin(&vkey[n], (u64)k);
        }
    }
}

// Reads vkey, key, dir and the connectivity; writes remap, Q and lock only on the vertices of its own ring, which no other
// winner of the pass shares and no lane of this kernel reads.
__global__ __launch_bounds__(256) void select_kernel(Conn m, const int64_t* __restrict__ key,
                                                     const int64_t* __restrict__ threshold, const int* __restrict__ dir,
                                                     const u64* __restrict__ vkey, int* __restrict__ remap,
                                                     double* __restrict__ Q, int* __restrict__ lock, int* __restrict__ flags)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m.E) return;
    const int64_t k = key[e];
    const int d = dir[e];
    if (!is_live(k, *threshold) || (d != 1 && d != 2)) return;
    const int lo = m.ev[2 * (size_t)e], hi = m.ev[2 * (size_t)e + 1];
    if (!in_range(lo, m.V) || !in_range(hi, m.V)) return;
    if (vkey[lo] != (u64)k || vkey[hi] != (u64)k) return;
    for (int s = 0; s < 2; s++) {
        const int v = s ? hi : lo;
        for (int i = m.nbr_ptr[v]; i < m.nbr_ptr[v + 1]; i++) {
            const int n = m.nbr_idx[i];
            if (in_range(n, m.V) && vkey[n] != (u64)k) return;
        }
    }
    const int a = d == 1 ? lo : hi, b = d == 1 ? hi : lo;
    remap[a] = b;
#pragma unroll
    for (int i = 0; i < 10; i++) Q[10 * (size_t)b + i] = Q[10 * (size_t)b + i] + Q[10 * (size_t)a + i];
    lock[lo] = 1;
    lock[hi] = 1;
    for (int s = 0; s < 2; s++) {
        const int v = s ? hi : lo;
        for (int i = m.nbr_ptr[v]; i < m.nbr_ptr[v + 1]; i++) {
            const int n = m.nbr_idx[i];
            if (in_range(n, m.V)) lock[n] = 1;
        }
    }
    atomicAdd(&flags[GD_REMESH_FLAG_SELECTED], 1);
}

// ---- smoothing and rotation -----------------------------------------------------------------------------------------------

// is (a, b) a boundary edge?  ev is sorted by (lo, hi)
__device__ bool boundary_edge(const Conn& m, int a, int b)
{
    const int lo = min(a, b), hi = max(a, b);
    int l = 0, r = m.E;
    while (l < r) {
        const int mid = l + (r - l) / 2;
        const int x = m.ev[2 * (size_t)mid], y = m.ev[2 * (size_t)mid + 1];
        if (x < lo || (x == lo && y < hi)) l = mid + 1;
        else r = mid;
    }
    return l < m.E && m.ev[2 * (size_t)l] == lo && m.ev[2 * (size_t)l + 1] == hi && m.eh[2 * (size_t)l + 1] < 0;
}

__global__ __launch_bounds__(256) void smooth_kernel(Conn m, float w, float* __restrict__ out)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= m.V) return;
    const float px = m.verts[3 * (size_t)v], py = m.verts[3 * (size_t)v + 1], pz = m.verts[3 * (size_t)v + 2];
    const bool rim = m.bnd[v] != 0;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    int k = 0;
    for (int j = m.nbr_ptr[v]; j < m.nbr_ptr[v + 1]; j++) {
        const int n = m.nbr_idx[j];
        if (!in_range(n, m.V) || (rim && !boundary_edge(m, v, n))) continue;
        sx = sx + m.verts[3 * (size_t)n];
        sy = sy + m.verts[3 * (size_t)n + 1];
        sz = sz + m.verts[3 * (size_t)n + 2];
        k++;
    }
    float ox = px, oy = py, oz = pz;
    if (k) {
        const float count = (float)k;
        ox = px + w * (sx / count - px);
        oy = py + w * (sy / count - py);
        oz = pz + w * (sz / count - pz);
    }
    out[3 * (size_t)v] = ox;
    out[3 * (size_t)v + 1] = oy;
    out[3 * (size_t)v + 2] = oz;
}

__global__ __launch_bounds__(256) void rotate_kernel(int V, const float* __restrict__ in, float* __restrict__ out)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const float x = in[3 * (size_t)v], y = in[3 * (size_t)v + 1], z = in[3 * (size_t)v + 2];
    out[3 * (size_t)v] = x;
    out[3 * (size_t)v + 1] = z;
    out[3 * (size_t)v + 2] = -y;
}

int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char buf[200];
        snprintf(buf, sizeof(buf), "simplify %s: %s", what, hipGetErrorString(e));
        return mesh_fail(-2, buf);
    }
    return 0;
}

dim3 grid_of(int n) { return dim3((unsigned)((max(n, 1) + 255) / 256)); }

constexpr int kMaxFaces = 1 << 29;   // 3F and every corner index stay below 2^31

bool mesh_ok(const gd_remesh_mesh* m)
{
    return m && m->V > 0 && m->F > 0 && m->F < kMaxFaces && m->E > 0 && m->E <= 3 * m->F && m->verts && m->tri && m->ev &&
           m->eh && m->bnd && m->nbr_ptr && m->nbr_idx && m->vf_ptr && m->vf_idx;
}

Conn conn_of(const gd_remesh_mesh* m)
{
    return Conn{m->V, m->F, m->E, m->verts, m->tri, m->ev, m->eh, m->bnd, m->nbr_ptr, m->nbr_idx, m->vf_ptr, m->vf_idx};
}

}  // namespace
}  // namespace gd

extern "C" {

using namespace gd;

int gd_mesh_simplify_quadrics(void* stream, const gd_remesh_mesh* mesh, double* Q)
{
    if (!mesh_ok(mesh) || !Q) return mesh_fail(-1, "simplify quadrics: bad arguments");
    hipLaunchKernelGGL(quadrics_kernel, grid_of(mesh->V), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), Q);
    return launched("quadrics");
}

int gd_mesh_simplify_candidates(void* stream, const gd_remesh_mesh* mesh, const double* Q, int64_t* key, int* dir,
                                double* cost)
{
    if (!mesh_ok(mesh) || !Q || !key || !dir || !cost) return mesh_fail(-1, "simplify candidates: bad arguments");
    hipLaunchKernelGGL(candidates_kernel, grid_of(mesh->E), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), Q, key, dir,
                       cost);
    return launched("candidates");
}

int gd_mesh_simplify_spread(void* stream, const gd_remesh_mesh* mesh, const int64_t* key, const int64_t* threshold,
                            const int* lock, uint64_t* vkey)
{
    if (!mesh_ok(mesh) || !key || !threshold || !lock || !vkey) return mesh_fail(-1, "simplify spread: bad arguments");
    hipLaunchKernelGGL(spread_kernel, grid_of(mesh->E), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), key, threshold,
                       lock, (u64*)vkey);
    return launched("spread");
}

int gd_mesh_simplify_select(void* stream, const gd_remesh_mesh* mesh, const int64_t* key, const int64_t* threshold,
                            const int* dir, const uint64_t* vkey, int* remap, double* Q, int* lock, int* flags)
{
    if (!mesh_ok(mesh) || !key || !threshold || !dir || !vkey || !remap || !Q || !lock || !flags)
        return mesh_fail(-1, "simplify select: bad arguments");
    hipLaunchKernelGGL(select_kernel, grid_of(mesh->E), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), key, threshold, dir,
                       (const u64*)vkey, remap, Q, lock, flags);
    return launched("select");
}

int gd_mesh_simplify_smooth(void* stream, const gd_remesh_mesh* mesh, float w, float* verts_out)
{
    if (!mesh_ok(mesh) || !verts_out || verts_out == mesh->verts || !(w == w))
        return mesh_fail(-1, "simplify smooth: bad arguments");
    hipLaunchKernelGGL(smooth_kernel, grid_of(mesh->V), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), w, verts_out);
    return launched("smooth");
}

int gd_mesh_simplify_rotate(void* stream, int V, const float* verts, float* verts_out)
{
    if (V <= 0 || !verts || !verts_out || verts == verts_out) return mesh_fail(-1, "simplify rotate: bad arguments");
    hipLaunchKernelGGL(rotate_kernel, grid_of(V), dim3(256), 0, (hipStream_t)stream, V, verts, verts_out);
    return launched("rotate");
}

}  // extern "C"
