// raster_remesh.hip -- isotropic remeshing of the deformer's mesh on the device (C-ABI and the DEFINITIONS:
// include/gd_mesh_remesh.h): connectivity from sorted keys, edge split, collapse and flip rounds selected by a minimum key,
// tangential relaxation and projection onto the surface the remesh started from through a uniform grid.  Built with
// -ffp-contract=off: the header fixes the order of every floating-point operation.
//
// Shape of every kernel: one lane per edge, face, vertex or sorted key; loops only over CSR ranges; rounds are separated by
// kernel boundaries, nothing waits across workgroups.  No floating-point atomics.  The integer atomics are plain HIP
// (atomicMin on 64-bit keys, atomicAdd / atomicOr on counters), device scope by default.  A kernel that writes through an
// index it read from a table checks it against the capacity it was given and raises GD_REMESH_FLAG_CAPACITY instead.
// The vector math, the connectivity tables (Conn), the two collapse tests shared with raster_simplify.hip and the ring
// walks (spread_key, holds_key) are in raster_mesh_common.h.
//
// A remesh runs once or twice per deformation on tens of thousands of faces: nothing here is tuned.  The scan is ONE
// workgroup that walks the array (no cross-workgroup carry to wait for); at 2*10^5 keys that is some 200 steps.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "raster_mesh_common.h"

namespace gd {
namespace {

constexpr u64 kNoKey = ~(u64)0;

__device__ __forceinline__ int lower_bound(const int64_t* __restrict__ keys, int n, int64_t x)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (keys[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// is x in the ascending idx[a, b)?
__device__ __forceinline__ bool contains(const int* __restrict__ idx, int a, int b, int x)
{
    while (a < b) {
        const int mid = a + (b - a) / 2;
        const int y = idx[mid];
        if (y == x) return true;
        if (y < x) a = mid + 1;
        else b = mid;
    }
    return false;
}

// ---- exclusive scan: one workgroup walks the array ------------------------------------------------------------------------

__global__ __launch_bounds__(1024) void scan_kernel(int n, const int* __restrict__ in, int* __restrict__ out)
{
    __shared__ int lds[1024];
    const int t = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + t;
        const int x = i < n ? in[i] : 0;
        lds[t] = x;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int y = t >= off ? lds[t - off] : 0;
            __syncthreads();
            lds[t] += y;
            __syncthreads();
        }
        if (i < n) out[i] = carry + lds[t] - x;
        carry += lds[1023];
        __syncthreads();
    }
    if (t == 0) out[n] = carry;
}

// ---- connectivity -------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void keys_kernel(int V, int F, const int* __restrict__ tri, int64_t* __restrict__ hkeys,
                                                   int64_t* __restrict__ ckeys, int* __restrict__ flags)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int v[3] = {tri[3 * (size_t)f], tri[3 * (size_t)f + 1], tri[3 * (size_t)f + 2]};
    if (!in_range(v[0], V) || !in_range(v[1], V) || !in_range(v[2], V)) {
        atomicOr(&flags[GD_REMESH_FLAG_INDEX], 1);
        v[0] = v[1] = v[2] = 0;
    } else if (v[0] == v[1] || v[1] == v[2] || v[2] == v[0]) {
        atomicOr(&flags[GD_REMESH_FLAG_REPEATED], 1);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int p = v[(i + 1) % 3], q = v[(i + 2) % 3];
        hkeys[3 * (size_t)f + i] = ((int64_t)min(p, q) << 32) | (int64_t)max(p, q);
        ckeys[3 * (size_t)f + i] = ((int64_t)v[i] << 32) | (int64_t)(3 * f + i);
    }
}

__global__ __launch_bounds__(256) void heads_kernel(int n, const int64_t* __restrict__ sk, int* __restrict__ head,
                                                    int* __restrict__ flags)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    head[j] = (j == 0 || sk[j] != sk[j - 1]) ? 1 : 0;
    if (j >= 2 && sk[j] == sk[j - 2]) atomicOr(&flags[GD_REMESH_FLAG_NONMANIFOLD], 1);
}

__global__ __launch_bounds__(256) void edge_tables_kernel(int V, int n, int E, const int64_t* __restrict__ sk,
                                                          const int64_t* __restrict__ order, const int* __restrict__ ex,
                                                          int* __restrict__ fe, int* __restrict__ ev, int* __restrict__ eh,
                                                          int64_t* __restrict__ ukeys, int64_t* __restrict__ rkeys,
                                                          int* __restrict__ bnd, int* __restrict__ flags)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int64_t key = sk[j];
    const int h = (j == 0 || key != sk[j - 1]) ? 1 : 0;
    const int e = ex[j] + h - 1;
    const int64_t k = order[j];
    const int lo = (int)(key >> 32), hi = (int)(key & 0xffffffff);
    if (!in_range(e, E) || k < 0 || k >= n || !in_range(lo, V) || !in_range(hi, V)) {
        atomicOr(&flags[GD_REMESH_FLAG_CAPACITY], 1);
        return;
    }
    fe[k] = e;
    if (!h) return;
    int64_t second = -1;
    if (j + 1 < n && sk[j + 1] == key) second = order[j + 1];
    if (second >= n) {
        atomicOr(&flags[GD_REMESH_FLAG_CAPACITY], 1);
        return;
    }
    ev[2 * (size_t)e] = lo;
    ev[2 * (size_t)e + 1] = hi;
    eh[2 * (size_t)e] = (int)k;
    eh[2 * (size_t)e + 1] = (int)second;
    ukeys[e] = key;
    rkeys[e] = ((int64_t)hi << 32) | (int64_t)lo;
    if (second < 0) {   // every writer stores the same value
        bnd[lo] = 1;
        bnd[hi] = 1;
    }
}

// v in [0, V]: the CSR pointers are positions in the sorted keys; v < V also fills its rows
__global__ __launch_bounds__(256) void vertex_tables_kernel(int V, int F, int E, const int64_t* __restrict__ ukeys,
                                                            const int64_t* __restrict__ srkeys,
                                                            const int64_t* __restrict__ sckeys, int* __restrict__ nbr_ptr,
                                                            int* __restrict__ nbr_idx, int* __restrict__ vf_ptr,
                                                            int* __restrict__ vf_idx)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v > V) return;
    const int64_t x = (int64_t)v << 32, y = (int64_t)(v + 1) << 32;
    const int sF = lower_bound(ukeys, E, x), sR = lower_bound(srkeys, E, x), sC = lower_bound(sckeys, 3 * F, x);
    nbr_ptr[v] = sF + sR;
    vf_ptr[v] = sC;
    if (v == V) return;
    const int eF = lower_bound(ukeys, E, y), eR = lower_bound(srkeys, E, y), eC = lower_bound(sckeys, 3 * F, y);
    int o = sF + sR;   // <= 2E - (eF - sF) - (eR - sR): both lists hold E keys
    for (int j = sR; j < eR; j++) nbr_idx[o++] = (int)(srkeys[j] & 0xffffffff);   // the smaller neighbours, ascending
    for (int j = sF; j < eF; j++) nbr_idx[o++] = (int)(ukeys[j] & 0xffffffff);    // then the larger
    for (int j = sC; j < eC; j++) vf_idx[j] = (int)(sckeys[j] & 0xffffffff);
}

// ---- split --------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void split_mark_kernel(int V, int E, const float* __restrict__ verts,
                                                         const int* __restrict__ ev, float hi2, int* __restrict__ mark)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int a = ev[2 * (size_t)e], b = ev[2 * (size_t)e + 1];
    mark[e] = (in_range(a, V) && in_range(b, V) && sqlen(load3(verts, a), load3(verts, b)) > hi2) ? 1 : 0;
}

__global__ __launch_bounds__(256) void split_count_kernel(int F, int E, const int* __restrict__ fe,
                                                          const int* __restrict__ mark, int* __restrict__ count)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int c = 1;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int e = fe[3 * (size_t)f + i];
        if (in_range(e, E)) c += mark[e];
    }
    count[f] = c;
}

__device__ __forceinline__ void emit(int* __restrict__ out, int pos, int a, int b, int c)
{
    out[3 * (size_t)pos] = a;
    out[3 * (size_t)pos + 1] = b;
    out[3 * (size_t)pos + 2] = c;
}

// lanes [0, E): the midpoint of a marked edge; lanes [0, F): the 1 to 4 faces of a face
__global__ __launch_bounds__(256) void split_apply_kernel(int V, int F, int E, int Vcap, int Fcap,
                                                          const float* __restrict__ verts, const int* __restrict__ tri,
                                                          const int* __restrict__ ev, const int* __restrict__ fe,
                                                          const int* __restrict__ mark, const int* __restrict__ escan,
                                                          const int* __restrict__ fscan, float* __restrict__ verts_out,
                                                          int* __restrict__ tri_out, int* __restrict__ flags)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < E && mark[t]) {
        const int a = ev[2 * (size_t)t], b = ev[2 * (size_t)t + 1], m = V + escan[t];
        if (in_range(a, V) && in_range(b, V) && m >= V && m < Vcap) store3(verts_out, m, midpoint(load3(verts, a), load3(verts, b)));
        else atomicOr(&flags[GD_REMESH_FLAG_CAPACITY], 1);
    }
    if (t >= F) return;
    int v[3], m[3], nm = 0;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        v[i] = tri[3 * (size_t)t + i];
        const int e = fe[3 * (size_t)t + i];
        ok = ok && in_range(v[i], V) && in_range(e, E);
        m[i] = -1;
        if (ok && mark[e]) {
            m[i] = V + escan[e];
            ok = ok && m[i] >= V && m[i] < Vcap;
            nm++;
        }
    }
    const int pos = fscan[t];
    if (!ok || pos < 0 || pos + nm + 1 > Fcap) {
        atomicOr(&flags[GD_REMESH_FLAG_CAPACITY], 1);
        return;
    }
    if (nm == 0) {
        emit(tri_out, pos, v[0], v[1], v[2]);
    } else if (nm == 1) {
        const int i = m[0] >= 0 ? 0 : (m[1] >= 0 ? 1 : 2);   // the marked edge lies opposite corner i = a
        const int a = v[i], b = v[(i + 1) % 3], c = v[(i + 2) % 3];
        emit(tri_out, pos, a, b, m[i]);
        emit(tri_out, pos + 1, a, m[i], c);
    } else if (nm == 2) {
        const int i = m[0] < 0 ? 0 : (m[1] < 0 ? 1 : 2);     // the unmarked edge lies opposite corner i = a
        const int a = v[i], b = v[(i + 1) % 3], c = v[(i + 2) % 3];
        const int mca = m[(i + 1) % 3], mab = m[(i + 2) % 3];
        const V3 pa = load3(verts, a), pb = load3(verts, b), pc = load3(verts, c);
        const float d_b = sqlen(pb, midpoint(pc, pa));       // diagonal b - mca
        const float d_c = sqlen(midpoint(pa, pb), pc);       // diagonal mab - c
        emit(tri_out, pos, a, mab, mca);
        if (d_b <= d_c) {
            emit(tri_out, pos + 1, mab, b, mca);
            emit(tri_out, pos + 2, b, c, mca);
        } else {
            emit(tri_out, pos + 1, mab, b, c);
            emit(tri_out, pos + 2, mab, c, mca);
        }
    } else {
        emit(tri_out, pos, v[0], m[2], m[1]);
        emit(tri_out, pos + 1, v[1], m[0], m[2]);
        emit(tri_out, pos + 2, v[2], m[1], m[0]);
        emit(tri_out, pos + 3, m[0], m[1], m[2]);
    }
}

// ---- collapse -----------------------------------------------------------------------------------------------------------

// the remesher's rules: a boundary vertex moves only along the boundary, the link condition, no edge longer than hi
__device__ bool collapse_allowed(const Conn& m, int a, int b, bool interior, float hi2)
{
    if (m.bnd[a] && interior) return false;
    if (m.bnd[a] && m.bnd[b] && interior) return false;
    int opposite[2];
    if (common_neighbours(m, a, b, opposite) != (interior ? 2 : 1)) return false;
    const V3 pb = load3(m.verts, b);
    for (int i = m.nbr_ptr[a]; i < m.nbr_ptr[a + 1]; i++) {
        const int n = m.nbr_idx[i];
        if (n == b || !in_range(n, m.V)) continue;
        if (sqlen(load3(m.verts, n), pb) > hi2) return false;
    }
    return collapse_keeps_normals<float>(m, a, b);
}

__global__ __launch_bounds__(256) void collapse_candidates_kernel(Conn m, float lo2, float hi2, int* __restrict__ dir,
                                                                  u64* __restrict__ ekey, u64* __restrict__ vkey)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m.E) return;
    const int lo = m.ev[2 * (size_t)e], hi = m.ev[2 * (size_t)e + 1];
    int d = 0;
    u64 key = kNoKey;
    if (in_range(lo, m.V) && in_range(hi, m.V) && lo != hi) {
        const float len2 = sqlen(load3(m.verts, lo), load3(m.verts, hi));
        if (len2 < lo2) {
            const bool interior = m.eh[2 * (size_t)e + 1] >= 0;
            const int k0 = m.eh[2 * (size_t)e];
            const int opposite = in_range(k0, 3 * m.F) ? m.tri[k0] : -1;
            if (!in_range(opposite, m.V) || (!interior && m.bnd[opposite])) {
                // a face with all three vertices on the boundary stays: no corner or ear of the surface is eaten
            } else if (collapse_allowed(m, lo, hi, interior, hi2)) d = 1;   // remove lo, keep hi
            else if (collapse_allowed(m, hi, lo, interior, hi2)) d = 2;   // remove hi, keep lo
            if (d) {
                key = ((u64)__float_as_uint(len2) << 32) | (u64)(unsigned)e;
                spread_key(m, lo, hi, key, vkey);
            }
        }
    }
    dir[e] = d;
    ekey[e] = key;
}

__global__ __launch_bounds__(256) void collapse_select_kernel(Conn m, const int* __restrict__ dir,
                                                              const u64* __restrict__ ekey, const u64* __restrict__ vkey,
                                                              int* __restrict__ remap, int* __restrict__ flags)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m.E || dir[e] == 0) return;
    const int lo = m.ev[2 * (size_t)e], hi = m.ev[2 * (size_t)e + 1];
    if (!in_range(lo, m.V) || !in_range(hi, m.V)) return;
    if (!holds_key(m, lo, hi, ekey[e], vkey)) return;
    if (dir[e] == 1) remap[lo] = hi;
    else remap[hi] = lo;
    atomicAdd(&flags[GD_REMESH_FLAG_SELECTED], 1);
}

__global__ __launch_bounds__(256) void relabel_kernel(int V, int F, const int* __restrict__ tri, const int* __restrict__ remap,
                                                      int* __restrict__ tri_out, int* __restrict__ alive,
                                                      int* __restrict__ flags)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int v[3];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        v[i] = tri[3 * (size_t)f + i];
        ok = ok && in_range(v[i], V);
        if (ok) v[i] = remap[v[i]];
        ok = ok && in_range(v[i], V);
    }
    if (!ok) {
        atomicOr(&flags[GD_REMESH_FLAG_CAPACITY], 1);
        alive[f] = 0;
        return;
    }
    emit(tri_out, f, v[0], v[1], v[2]);
    alive[f] = (v[0] != v[1] && v[1] != v[2] && v[2] != v[0]) ? 1 : 0;
}

__global__ __launch_bounds__(256) void compact_faces_kernel(int F, int Fcap, const int* __restrict__ tri,
                                                            const int* __restrict__ alive, const int* __restrict__ scan,
                                                            int* __restrict__ tri_out, int* __restrict__ flags)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F || !alive[f]) return;
    const int pos = scan[f];
    if (!in_range(pos, Fcap)) {
        atomicOr(&flags[GD_REMESH_FLAG_CAPACITY], 1);
        return;
    }
    emit(tri_out, pos, tri[3 * (size_t)f], tri[3 * (size_t)f + 1], tri[3 * (size_t)f + 2]);
}

// ---- flip ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int valence_cost(const Conn& m, int v, int change)
{
    return abs(m.nbr_ptr[v + 1] - m.nbr_ptr[v] + change - (m.bnd[v] ? 4 : 6));
}

// quad[e] = (c, p, q, d): faces (c, p, q) and (d, q, p) become (c, p, d) and (c, d, q); c = -1: no candidate
__global__ __launch_bounds__(256) void flip_candidates_kernel(Conn m, int4* __restrict__ quad, u64* __restrict__ ekey,
                                                              u64* __restrict__ vkey)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m.E) return;
    int4 out = make_int4(-1, -1, -1, -1);
    u64 key = kNoKey;
    const int k0 = m.eh[2 * (size_t)e], k1 = m.eh[2 * (size_t)e + 1];
    if (in_range(k0, 3 * m.F) && in_range(k1, 3 * m.F)) {
        const int f0 = k0 / 3, i0 = k0 - 3 * f0, f1 = k1 / 3, i1 = k1 - 3 * f1;
        const int c = m.tri[3 * (size_t)f0 + i0], p = m.tri[3 * (size_t)f0 + (i0 + 1) % 3], q = m.tri[3 * (size_t)f0 + (i0 + 2) % 3];
        const int d = m.tri[3 * (size_t)f1 + i1], p1 = m.tri[3 * (size_t)f1 + (i1 + 1) % 3], q1 = m.tri[3 * (size_t)f1 + (i1 + 2) % 3];
        const bool valid = in_range(c, m.V) && in_range(p, m.V) && in_range(q, m.V) && in_range(d, m.V) && f0 != f1 &&
                           p1 == q && q1 == p && c != d && c != p && c != q && d != p && d != q && p != q;
        if (valid && !contains(m.nbr_idx, m.nbr_ptr[c], m.nbr_ptr[c + 1], d)) {
            const int before = valence_cost(m, p, 0) + valence_cost(m, q, 0) + valence_cost(m, c, 0) + valence_cost(m, d, 0);
            const int after = valence_cost(m, p, -1) + valence_cost(m, q, -1) + valence_cost(m, c, 1) + valence_cost(m, d, 1);
            if (after < before) {
                const V3 pc = load3(m.verts, c), pp = load3(m.verts, p), pq = load3(m.verts, q), pd = load3(m.verts, d);
                const V3 n0 = tri_normal(pc, pp, pq), n1 = tri_normal(pd, pq, pp);
                const V3 m0 = tri_normal(pc, pp, pd), m1 = tri_normal(pc, pd, pq);
                if (dot(m0, n0) > 0.0f && dot(m0, n1) > 0.0f && dot(m1, n0) > 0.0f && dot(m1, n1) > 0.0f) {
                    out = make_int4(c, p, q, d);
                    key = ((u64)(unsigned)(after - before + 0x40000000) << 32) | (u64)(unsigned)e;
                    atomicMin(&vkey[c], key);
                    atomicMin(&vkey[p], key);
                    atomicMin(&vkey[q], key);
                    atomicMin(&vkey[d], key);
                }
            }
        }
    }
    quad[e] = out;
    ekey[e] = key;
}

// reads only quad / ekey / vkey / eh, so that no lane reads a face another lane rewrites
__global__ __launch_bounds__(256) void flip_apply_kernel(int V, int F, int E, const int* __restrict__ eh,
                                                         const int4* __restrict__ quad, const u64* __restrict__ ekey,
                                                         const u64* __restrict__ vkey, int* __restrict__ tri,
                                                         int* __restrict__ flags)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int4 g = quad[e];
    const u64 key = ekey[e];
    if (g.x < 0 || key == kNoKey) return;
    if (!in_range(g.x, V) || !in_range(g.y, V) || !in_range(g.z, V) || !in_range(g.w, V)) {
        atomicOr(&flags[GD_REMESH_FLAG_CAPACITY], 1);
        return;
    }
    if (vkey[g.x] != key || vkey[g.y] != key || vkey[g.z] != key || vkey[g.w] != key) return;
    const int k0 = eh[2 * (size_t)e], k1 = eh[2 * (size_t)e + 1];
    if (!in_range(k0, 3 * F) || !in_range(k1, 3 * F)) {
        atomicOr(&flags[GD_REMESH_FLAG_CAPACITY], 1);
        return;
    }
    emit(tri, k0 / 3, g.x, g.y, g.w);
    emit(tri, k1 / 3, g.x, g.w, g.z);
    atomicAdd(&flags[GD_REMESH_FLAG_SELECTED], 1);
}

// ---- relax --------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void relax_kernel(Conn m, float* __restrict__ out, int* __restrict__ moved)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= m.V) return;
    const V3 p = load3(m.verts, v);
    const int a = m.nbr_ptr[v], b = m.nbr_ptr[v + 1];
    if (m.bnd[v] || b <= a) {
        store3(out, v, p);
        moved[v] = 0;
        return;
    }
    V3 s = V3{0.0f, 0.0f, 0.0f};
    for (int j = a; j < b; j++) {
        const int k = m.nbr_idx[j];
        if (in_range(k, m.V)) s = add(s, load3(m.verts, k));
    }
    const float deg = (float)(b - a);
    const V3 d = sub(V3{s.x / deg, s.y / deg, s.z / deg}, p);
    V3 n = V3{0.0f, 0.0f, 0.0f};
    for (int j = m.vf_ptr[v]; j < m.vf_ptr[v + 1]; j++) {
        const int corner = m.vf_idx[j];
        if (!in_range(corner, 3 * m.F)) continue;
        const int f = corner / 3;
        const int x0 = m.tri[3 * (size_t)f], x1 = m.tri[3 * (size_t)f + 1], x2 = m.tri[3 * (size_t)f + 2];
        if (in_range(x0, m.V) && in_range(x1, m.V) && in_range(x2, m.V))
            n = add(n, tri_normal(load3(m.verts, x0), load3(m.verts, x1), load3(m.verts, x2)));
    }
    const float l = fmaxf(sqrtf(dot(n, n)), kNormEps);
    n = V3{n.x / l, n.y / l, n.z / l};
    const float t = dot(n, d);
    store3(out, v, V3{p.x + (d.x - n.x * t), p.y + (d.y - n.y * t), p.z + (d.z - n.z * t)});
    moved[v] = 1;
}

// ---- projection ---------------------------------------------------------------------------------------------------------

struct Grid {
    float ox, oy, oz, c;
    int nx, ny, nz;
};

// the cell coordinate along one axis, not clamped to the grid but kept where the conversion is defined
__device__ __forceinline__ int cell_of(float x, float o, float c, int n)
{
    return (int)fminf(fmaxf(floorf((x - o) / c), -2.0f), (float)(n + 1));
}
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

__device__ __forceinline__ bool tri_cells(const Grid& g, int V, const float* __restrict__ verts, const int* __restrict__ tri,
                                          int f, int lo[3], int hi[3])
{
    const int x0 = tri[3 * (size_t)f], x1 = tri[3 * (size_t)f + 1], x2 = tri[3 * (size_t)f + 2];
    if (!in_range(x0, V) || !in_range(x1, V) || !in_range(x2, V)) return false;
    const V3 a = load3(verts, x0), b = load3(verts, x1), c = load3(verts, x2);
    lo[0] = clampi(cell_of(fminf(a.x, fminf(b.x, c.x)), g.ox, g.c, g.nx), 0, g.nx - 1);
    hi[0] = clampi(cell_of(fmaxf(a.x, fmaxf(b.x, c.x)), g.ox, g.c, g.nx), 0, g.nx - 1);
    lo[1] = clampi(cell_of(fminf(a.y, fminf(b.y, c.y)), g.oy, g.c, g.ny), 0, g.ny - 1);
    hi[1] = clampi(cell_of(fmaxf(a.y, fmaxf(b.y, c.y)), g.oy, g.c, g.ny), 0, g.ny - 1);
    lo[2] = clampi(cell_of(fminf(a.z, fminf(b.z, c.z)), g.oz, g.c, g.nz), 0, g.nz - 1);
    hi[2] = clampi(cell_of(fmaxf(a.z, fmaxf(b.z, c.z)), g.oz, g.c, g.nz), 0, g.nz - 1);
    return true;
}

// scatter == 0: count the triangles of each cell; else place them (start + a cursor that counts again)
__global__ __launch_bounds__(256) void grid_bin_kernel(Grid g, int V, int F, const float* __restrict__ verts,
                                                       const int* __restrict__ tri, int scatter, int* __restrict__ count,
                                                       const int* __restrict__ start, int* __restrict__ items, int cap,
                                                       int* __restrict__ flags)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int lo[3], hi[3];
    if (!tri_cells(g, V, verts, tri, f, lo, hi)) {
        atomicOr(&flags[GD_REMESH_FLAG_INDEX], 1);
        return;
    }
    for (int z = lo[2]; z <= hi[2]; z++)
        for (int y = lo[1]; y <= hi[1]; y++)
            for (int x = lo[0]; x <= hi[0]; x++) {
                const int cell = (z * g.ny + y) * g.nx + x;
                const int slot = atomicAdd(&count[cell], 1);
                if (!scatter) continue;
                const int pos = start[cell] + slot;
                if (in_range(pos, cap)) items[pos] = f;
                else atomicOr(&flags[GD_REMESH_FLAG_CAPACITY], 1);
            }
}

// the closest point of triangle (a, b, c) to p: the region tests of the header
__device__ V3 closest_on_triangle(V3 p, V3 a, V3 b, V3 c)
{
    const V3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a);
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0f && d2 <= 0.0f) return a;
    const V3 bp = sub(p, b);
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0f && d4 <= d3) return b;
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) return add(a, scale(ab, d1 / (d1 - d3)));
    const V3 cp = sub(p, c);
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0f && d5 <= d6) return c;
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) return add(a, scale(ac, d2 / (d2 - d6)));
    const float va = d3 * d6 - d5 * d4;
    if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f)
        return add(b, scale(sub(c, b), (d4 - d3) / ((d4 - d3) + (d5 - d6))));
    const float s = (va + vb) + vc;
    return add(add(a, scale(ab, vb / s)), scale(ac, vc / s));
}

__global__ __launch_bounds__(256) void project_kernel(Grid g, int n, const float* __restrict__ q, const int* __restrict__ moved,
                                                      int V, int F, const float* __restrict__ verts,
                                                      const int* __restrict__ tri, const int* __restrict__ start,
                                                      const int* __restrict__ items, int cap, float* __restrict__ out,
                                                      int* __restrict__ flags)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const V3 p = load3(q, v);
    if (moved && !moved[v]) {
        store3(out, v, p);
        return;
    }
    const int cx = cell_of(p.x, g.ox, g.c, g.nx), cy = cell_of(p.y, g.oy, g.c, g.ny), cz = cell_of(p.z, g.oz, g.c, g.nz);
    float best = INFINITY;
    int best_f = 0x7fffffff;
    V3 best_p = p;
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.nz - 1); z++)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.ny - 1); y++)
            for (int x = max(cx - 1, 0); x <= min(cx + 1, g.nx - 1); x++) {
                const int cell = (z * g.ny + y) * g.nx + x;
                const int j0 = max(start[cell], 0), j1 = min(start[cell + 1], cap);
                for (int j = j0; j < j1; j++) {
                    const int f = items[j];
                    if (!in_range(f, F)) continue;
                    const int x0 = tri[3 * (size_t)f], x1 = tri[3 * (size_t)f + 1], x2 = tri[3 * (size_t)f + 2];
                    if (!in_range(x0, V) || !in_range(x1, V) || !in_range(x2, V)) continue;
                    const V3 r = closest_on_triangle(p, load3(verts, x0), load3(verts, x1), load3(verts, x2));
                    const float d2 = sqlen(r, p);
                    if (d2 < best || (d2 == best && f < best_f)) {
                        best = d2;
                        best_f = f;
                        best_p = r;
                    }
                }
            }
    if (best <= g.c * g.c) {
        store3(out, v, best_p);
    } else {
        store3(out, v, p);
        atomicAdd(&flags[GD_REMESH_FLAG_UNPROJECTED], 1);
    }
}

// ---- vertex compaction and edge lengths ------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void used_vertices_kernel(int V, int F, const int* __restrict__ tri, int* __restrict__ used,
                                                            int* __restrict__ flags)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int v = tri[3 * (size_t)f + i];
        if (in_range(v, V)) used[v] = 1;   // every writer stores the same value
        else atomicOr(&flags[GD_REMESH_FLAG_INDEX], 1);
    }
}

__global__ __launch_bounds__(256) void compact_vertices_kernel(int V, int F, int Vcap, const float* __restrict__ verts,
                                                               const int* __restrict__ tri, const int* __restrict__ used,
                                                               const int* __restrict__ scan, float* __restrict__ verts_out,
                                                               int* __restrict__ tri_out, int* __restrict__ flags)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < V && used[t]) {
        if (in_range(scan[t], Vcap)) store3(verts_out, scan[t], load3(verts, t));
        else atomicOr(&flags[GD_REMESH_FLAG_CAPACITY], 1);
    }
    if (t >= F) return;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int v = tri[3 * (size_t)t + i];
        const int w = in_range(v, V) ? scan[v] : -1;
        if (in_range(w, Vcap)) tri_out[3 * (size_t)t + i] = w;
        else {
            tri_out[3 * (size_t)t + i] = 0;
            atomicOr(&flags[GD_REMESH_FLAG_CAPACITY], 1);
        }
    }
}

__global__ __launch_bounds__(256) void edge_lengths_kernel(int V, int E, const float* __restrict__ verts,
                                                           const int64_t* __restrict__ edges, float* __restrict__ len)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t a = edges[2 * (size_t)e], b = edges[2 * (size_t)e + 1];
    len[e] = (a >= 0 && a < V && b >= 0 && b < V) ? sqrtf(sqlen(load3(verts, a), load3(verts, b))) : 0.0f;
}

bool sizes_ok(int V, int F, int E) { return V > 0 && F >= 0 && F < kMaxFaces && E >= 0 && E <= 3 * F; }

bool grid_ok(const gd_remesh_grid* g)
{
    return g && g->cell > 0.0f && isfinite(g->cell) && isfinite(g->origin[0]) && isfinite(g->origin[1]) &&
           isfinite(g->origin[2]) && g->dims[0] > 0 && g->dims[1] > 0 && g->dims[2] > 0 &&
           (int64_t)g->dims[0] * g->dims[1] * g->dims[2] <= GD_REMESH_MAX_CELLS;
}

Grid grid_of_c(const gd_remesh_grid* g)
{
    return Grid{g->origin[0], g->origin[1], g->origin[2], g->cell, g->dims[0], g->dims[1], g->dims[2]};
}

}  // namespace
}  // namespace gd

extern "C" {

using namespace gd;

int gd_mesh_remesh_scan(void* stream, int n, const int* in, int* out)
{
    if (n < 0 || !out || (n > 0 && !in) || in == out) return mesh_fail(-1, "remesh scan: bad arguments");
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, n, in, out);
    return mesh_launched("remesh", "scan");
}

int gd_mesh_remesh_keys(void* stream, int V, int F, const int* tri, int64_t* hkeys, int64_t* ckeys, int* flags)
{
    if (!sizes_ok(V, F, 0) || F == 0 || !tri || !hkeys || !ckeys || !flags) return mesh_fail(-1, "remesh keys: bad arguments");
    hipLaunchKernelGGL(keys_kernel, grid_of(F), dim3(256), 0, (hipStream_t)stream, V, F, tri, hkeys, ckeys, flags);
    return mesh_launched("remesh", "keys");
}

int gd_mesh_remesh_heads(void* stream, int n, const int64_t* sorted_keys, int* head, int* flags)
{
    if (n <= 0 || !sorted_keys || !head || !flags) return mesh_fail(-1, "remesh heads: bad arguments");
    hipLaunchKernelGGL(heads_kernel, grid_of(n), dim3(256), 0, (hipStream_t)stream, n, sorted_keys, head, flags);
    return mesh_launched("remesh", "heads");
}

int gd_mesh_remesh_edge_tables(void* stream, int V, int F, int E, const int64_t* sorted_keys, const int64_t* order,
                               const int* head_scan, int* fe, int* ev, int* eh, int64_t* ukeys, int64_t* rkeys, int* bnd,
                               int* flags)
{
    if (!sizes_ok(V, F, E) || F == 0 || E == 0 || !sorted_keys || !order || !head_scan || !fe || !ev || !eh || !ukeys ||
        !rkeys || !bnd || !flags)
        return mesh_fail(-1, "remesh edge tables: bad arguments");
    hipLaunchKernelGGL(edge_tables_kernel, grid_of(3 * F), dim3(256), 0, (hipStream_t)stream, V, 3 * F, E, sorted_keys, order,
                       head_scan, fe, ev, eh, ukeys, rkeys, bnd, flags);
    return mesh_launched("remesh", "edge tables");
}

int gd_mesh_remesh_vertex_tables(void* stream, int V, int F, int E, const int64_t* ukeys, const int64_t* sorted_rkeys,
                                 const int64_t* sorted_ckeys, int* nbr_ptr, int* nbr_idx, int* vf_ptr, int* vf_idx)
{
    if (!sizes_ok(V, F, E) || F == 0 || E == 0 || !ukeys || !sorted_rkeys || !sorted_ckeys || !nbr_ptr || !nbr_idx ||
        !vf_ptr || !vf_idx)
        return mesh_fail(-1, "remesh vertex tables: bad arguments");
    hipLaunchKernelGGL(vertex_tables_kernel, grid_of(V + 1), dim3(256), 0, (hipStream_t)stream, V, F, E, ukeys, sorted_rkeys,
                       sorted_ckeys, nbr_ptr, nbr_idx, vf_ptr, vf_idx);
    return mesh_launched("remesh", "vertex tables");
}

int gd_mesh_remesh_split_mark(void* stream, int V, int E, const float* verts, const int* ev, float hi2, int* mark)
{
    if (V <= 0 || E <= 0 || !verts || !ev || !mark || !(hi2 > 0.0f)) return mesh_fail(-1, "remesh split mark: bad arguments");
    hipLaunchKernelGGL(split_mark_kernel, grid_of(E), dim3(256), 0, (hipStream_t)stream, V, E, verts, ev, hi2, mark);
    return mesh_launched("remesh", "split mark");
}

int gd_mesh_remesh_split_count(void* stream, int F, int E, const int* fe, const int* mark, int* count)
{
    if (F <= 0 || E <= 0 || !fe || !mark || !count) return mesh_fail(-1, "remesh split count: bad arguments");
    hipLaunchKernelGGL(split_count_kernel, grid_of(F), dim3(256), 0, (hipStream_t)stream, F, E, fe, mark, count);
    return mesh_launched("remesh", "split count");
}

int gd_mesh_remesh_split_apply(void* stream, int V, int F, int E, int Vcap, int Fcap, const float* verts, const int* tri,
                               const int* ev, const int* fe, const int* mark, const int* edge_scan, const int* face_scan,
                               float* verts_out, int* tri_out, int* flags)
{
    if (!sizes_ok(V, F, E) || F == 0 || E == 0 || Vcap < V || Fcap < F || Fcap >= kMaxFaces || !verts || !tri || !ev || !fe ||
        !mark || !edge_scan || !face_scan || !verts_out || !tri_out || !flags)
        return mesh_fail(-1, "remesh split apply: bad arguments");
    hipLaunchKernelGGL(split_apply_kernel, grid_of(max(E, F)), dim3(256), 0, (hipStream_t)stream, V, F, E, Vcap, Fcap, verts,
                       tri, ev, fe, mark, edge_scan, face_scan, verts_out, tri_out, flags);
    return mesh_launched("remesh", "split apply");
}

int gd_mesh_remesh_collapse_candidates(void* stream, const gd_remesh_mesh* mesh, float lo2, float hi2, int* dir,
                                       uint64_t* ekey, uint64_t* vkey)
{
    if (!mesh_ok(mesh, false) || mesh->E == 0 || !dir || !ekey || !vkey || !(lo2 > 0.0f) || !(hi2 > 0.0f))
        return mesh_fail(-1, "remesh collapse candidates: bad arguments");
    hipLaunchKernelGGL(collapse_candidates_kernel, grid_of(mesh->E), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), lo2,
                       hi2, dir, (u64*)ekey, (u64*)vkey);
    return mesh_launched("remesh", "collapse candidates");
}

int gd_mesh_remesh_collapse_select(void* stream, const gd_remesh_mesh* mesh, const int* dir, const uint64_t* ekey,
                                   const uint64_t* vkey, int* remap, int* flags)
{
    if (!mesh_ok(mesh, false) || mesh->E == 0 || !dir || !ekey || !vkey || !remap || !flags)
        return mesh_fail(-1, "remesh collapse select: bad arguments");
    hipLaunchKernelGGL(collapse_select_kernel, grid_of(mesh->E), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), dir,
                       (const u64*)ekey, (const u64*)vkey, remap, flags);
    return mesh_launched("remesh", "collapse select");
}

int gd_mesh_remesh_relabel(void* stream, int V, int F, const int* tri, const int* remap, int* tri_out, int* alive, int* flags)
{
    if (!sizes_ok(V, F, 0) || F == 0 || !tri || !remap || !tri_out || !alive || !flags)
        return mesh_fail(-1, "remesh relabel: bad arguments");
    hipLaunchKernelGGL(relabel_kernel, grid_of(F), dim3(256), 0, (hipStream_t)stream, V, F, tri, remap, tri_out, alive, flags);
    return mesh_launched("remesh", "relabel");
}

int gd_mesh_remesh_compact_faces(void* stream, int F, int Fcap, const int* tri, const int* alive, const int* alive_scan,
                                 int* tri_out, int* flags)
{
    if (F <= 0 || F >= kMaxFaces || Fcap < 0 || !tri || !alive || !alive_scan || !flags || (Fcap > 0 && !tri_out))
        return mesh_fail(-1, "remesh compact faces: bad arguments");
    hipLaunchKernelGGL(compact_faces_kernel, grid_of(F), dim3(256), 0, (hipStream_t)stream, F, Fcap, tri, alive, alive_scan,
                       tri_out, flags);
    return mesh_launched("remesh", "compact faces");
}

int gd_mesh_remesh_flip_candidates(void* stream, const gd_remesh_mesh* mesh, int* quad, uint64_t* ekey, uint64_t* vkey)
{
    if (!mesh_ok(mesh, false) || mesh->E == 0 || !quad || !ekey || !vkey) return mesh_fail(-1, "remesh flip candidates: bad arguments");
    hipLaunchKernelGGL(flip_candidates_kernel, grid_of(mesh->E), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), (int4*)quad,
                       (u64*)ekey, (u64*)vkey);
    return mesh_launched("remesh", "flip candidates");
}

int gd_mesh_remesh_flip_apply(void* stream, int V, int F, int E, const int* eh, const int* quad, const uint64_t* ekey,
                              const uint64_t* vkey, int* tri, int* flags)
{
    if (!sizes_ok(V, F, E) || E == 0 || !eh || !quad || !ekey || !vkey || !tri || !flags)
        return mesh_fail(-1, "remesh flip apply: bad arguments");
    hipLaunchKernelGGL(flip_apply_kernel, grid_of(E), dim3(256), 0, (hipStream_t)stream, V, F, E, eh, (const int4*)quad,
                       (const u64*)ekey, (const u64*)vkey, tri, flags);
    return mesh_launched("remesh", "flip apply");
}

int gd_mesh_remesh_relax(void* stream, const gd_remesh_mesh* mesh, float* verts_out, int* moved)
{
    if (!mesh_ok(mesh, false) || !verts_out || !moved || verts_out == mesh->verts)
        return mesh_fail(-1, "remesh relax: bad arguments");
    hipLaunchKernelGGL(relax_kernel, grid_of(mesh->V), dim3(256), 0, (hipStream_t)stream, conn_of(mesh), verts_out, moved);
    return mesh_launched("remesh", "relax");
}

int gd_mesh_remesh_grid_bin(void* stream, const gd_remesh_grid* grid, int V, int F, const float* verts, const int* tri,
                            int scatter, int* count, const int* start, int* items, int capacity, int* flags)
{
    if (!grid_ok(grid) || !sizes_ok(V, F, 0) || F == 0 || !verts || !tri || !count || !flags ||
        (scatter && (!start || !items || capacity <= 0)))
        return mesh_fail(-1, "remesh grid: bad arguments");
    hipLaunchKernelGGL(grid_bin_kernel, grid_of(F), dim3(256), 0, (hipStream_t)stream, grid_of_c(grid), V, F, verts, tri,
                       scatter, count, start, items, capacity, flags);
    return mesh_launched("remesh", "grid");
}

int gd_mesh_remesh_project(void* stream, const gd_remesh_grid* grid, int n, const float* points, const int* moved, int V,
                           int F, const float* verts, const int* tri, const int* start, const int* items, int capacity,
                           float* out, int* flags)
{
    if (!grid_ok(grid) || n <= 0 || !sizes_ok(V, F, 0) || F == 0 || !points || !verts || !tri || !start || !items ||
        capacity <= 0 || !out || !flags)
        return mesh_fail(-1, "remesh project: bad arguments");
    hipLaunchKernelGGL(project_kernel, grid_of(n), dim3(256), 0, (hipStream_t)stream, grid_of_c(grid), n, points, moved, V, F,
                       verts, tri, start, items, capacity, out, flags);
    return mesh_launched("remesh", "project");
}

int gd_mesh_remesh_used_vertices(void* stream, int V, int F, const int* tri, int* used, int* flags)
{
    if (!sizes_ok(V, F, 0) || F == 0 || !tri || !used || !flags) return mesh_fail(-1, "remesh used vertices: bad arguments");
    hipLaunchKernelGGL(used_vertices_kernel, grid_of(F), dim3(256), 0, (hipStream_t)stream, V, F, tri, used, flags);
    return mesh_launched("remesh", "used vertices");
}

int gd_mesh_remesh_compact_vertices(void* stream, int V, int F, int Vcap, const float* verts, const int* tri, const int* used,
                                    const int* used_scan, float* verts_out, int* tri_out, int* flags)
{
    if (!sizes_ok(V, F, 0) || F == 0 || Vcap <= 0 || !verts || !tri || !used || !used_scan || !verts_out || !tri_out || !flags)
        return mesh_fail(-1, "remesh compact vertices: bad arguments");
    hipLaunchKernelGGL(compact_vertices_kernel, grid_of(max(V, F)), dim3(256), 0, (hipStream_t)stream, V, F, Vcap, verts, tri,
                       used, used_scan, verts_out, tri_out, flags);
    return mesh_launched("remesh", "compact vertices");
}

int gd_mesh_remesh_edge_lengths(void* stream, int V, int E, const float* verts, const int64_t* edges, float* len)
{
    if (V <= 0 || E <= 0 || !verts || !edges || !len) return mesh_fail(-1, "remesh edge lengths: bad arguments");
    hipLaunchKernelGGL(edge_lengths_kernel, grid_of(E), dim3(256), 0, (hipStream_t)stream, V, E, verts, edges, len);
    return mesh_launched("remesh", "edge lengths");
}

}  // extern "C"
