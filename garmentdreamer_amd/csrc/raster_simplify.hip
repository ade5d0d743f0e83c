// raster_simplify.hip -- the deformer's final-mesh post-process on the device (C-ABI and the DEFINITIONS:
// include/gd_mesh_simplify.h): quadric-error decimation by half-edge collapses in rounds of independent sets, Taubin
// smoothing, and the rotation of the final mesh.  Built with -ffp-contract=off: the header fixes the order of every
// floating-point operation.  Quadrics, costs and the flip test are fp64; smoothing is fp32.
//
// Shape of every kernel, as in raster_remesh.hip: one lane per edge or vertex, loops only over CSR ranges, passes separated
// by kernel boundaries.  The only atomics are atomicMin on 64-bit keys and atomicAdd on one counter.  Every index read from
// a table is checked against its range before it is used to read or write.  Conn, the fp64 vectors (D3), the link and
// normal tests of a collapse and the ring walks are those of raster_mesh_common.h.
//
// This runs once per deformation; nothing here is tuned.  The candidate kernel is bound by the divergence of its CSR rows
// and the spread kernel by scattered 8-byte atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/gd_mesh_simplify.h"
#include "raster_mesh_common.h"

namespace gd {
namespace {

constexpr int64_t kNoKey = INT64_MAX;

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
        const D3 p0 = load3<double>(m.verts, x0);
        const D3 n = tri_normal(p0, load3<double>(m.verts, x1), load3<double>(m.verts, x2));
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
    const D3 p = load3<double>(m.verts, b);
    const double squares = ((q[0] * p.x) * p.x + (q[4] * p.y) * p.y) + (q[7] * p.z) * p.z;
    const double mixed = ((q[1] * p.x) * p.y + (q[2] * p.x) * p.z) + (q[5] * p.y) * p.z;
    const double linear = (q[3] * p.x + q[6] * p.y) + q[8] * p.z;
    const double value = ((squares + 2.0 * mixed) + 2.0 * linear) + q[9];
    return value > 0.0 ? value : 0.0;
}

// the simplifier's rules: interior vertices only, the link condition, and no opposite vertex left with too few edges
__device__ bool collapse_allowed(const Conn& m, int a, int b)
{
    if (m.bnd[a]) return false;
    int opposite[2] = {-1, -1};
    if (common_neighbours(m, a, b, opposite) != 2) return false;
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int n = opposite[s];
        if (!in_range(n, m.V)) return false;
        if (!(m.nbr_ptr[n + 1] - m.nbr_ptr[n] > (m.bnd[n] ? 2 : 3))) return false;
    }
    return collapse_keeps_normals<double>(m, a, b);
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
    if (!for_each_ring_vertex(m, lo, hi, [lock](int v) { return !lock[v]; })) return;
    spread_key(m, lo, hi, (u64)k, vkey);
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
    if (!holds_key(m, lo, hi, (u64)k, vkey)) return;
    const int a = d == 1 ? lo : hi, b = d == 1 ? hi : lo;
    remap[a] = b;
#pragma unroll
    for (int i = 0; i < 10; i++) Q[10 * (size_t)b + i] = Q[10 * (size_t)b + i] + Q[10 * (size_t)a + i];
    for_each_ring_vertex(m, lo, hi, [lock](int v) {
        lock[v] = 1;
        return true;
    });
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

}  // namespace
}  // namespace gd

extern "C" {

using namespace gd;

int gd_mesh_simplify_quadrics(void* stream, const gd_remesh_mesh* mesh, double* Q)
{
    if (!mesh_ok(mesh, true) || !Q) return mesh_fail(-1, "simplify quadrics: bad arguments");
    hipLaunchKernelGGL(quadrics_kernel, grid_of(mesh->V), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), Q);
    return mesh_launched("simplify", "quadrics");
}

int gd_mesh_simplify_candidates(void* stream, const gd_remesh_mesh* mesh, const double* Q, int64_t* key, int* dir,
                                double* cost)
{
    if (!mesh_ok(mesh, true) || !Q || !key || !dir || !cost) return mesh_fail(-1, "simplify candidates: bad arguments");
    hipLaunchKernelGGL(candidates_kernel, grid_of(mesh->E), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), Q, key, dir,
                       cost);
    return mesh_launched("simplify", "candidates");
}

int gd_mesh_simplify_spread(void* stream, const gd_remesh_mesh* mesh, const int64_t* key, const int64_t* threshold,
                            const int* lock, uint64_t* vkey)
{
    if (!mesh_ok(mesh, true) || !key || !threshold || !lock || !vkey) return mesh_fail(-1, "simplify spread: bad arguments");
    hipLaunchKernelGGL(spread_kernel, grid_of(mesh->E), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), key, threshold,
                       lock, (u64*)vkey);
    return mesh_launched("simplify", "spread");
}

int gd_mesh_simplify_select(void* stream, const gd_remesh_mesh* mesh, const int64_t* key, const int64_t* threshold,
                            const int* dir, const uint64_t* vkey, int* remap, double* Q, int* lock, int* flags)
{
    if (!mesh_ok(mesh, true) || !key || !threshold || !dir || !vkey || !remap || !Q || !lock || !flags)
        return mesh_fail(-1, "simplify select: bad arguments");
    hipLaunchKernelGGL(select_kernel, grid_of(mesh->E), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), key, threshold, dir,
                       (const u64*)vkey, remap, Q, lock, flags);
    return mesh_launched("simplify", "select");
}

int gd_mesh_simplify_smooth(void* stream, const gd_remesh_mesh* mesh, float w, float* verts_out)
{
    if (!mesh_ok(mesh, true) || !verts_out || verts_out == mesh->verts || !(w == w))
        return mesh_fail(-1, "simplify smooth: bad arguments");
    hipLaunchKernelGGL(smooth_kernel, grid_of(mesh->V), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), w, verts_out);
    return mesh_launched("simplify", "smooth");
}

int gd_mesh_simplify_rotate(void* stream, int V, const float* verts, float* verts_out)
{
    if (V <= 0 || !verts || !verts_out || verts == verts_out) return mesh_fail(-1, "simplify rotate: bad arguments");
    hipLaunchKernelGGL(rotate_kernel, grid_of(V), dim3(256), 0, (hipStream_t)stream, V, verts, verts_out);
    return mesh_launched("simplify", "rotate");
}

}  // extern "C"
