// raster_clean.hip -- mesh cleaning (C-ABI and the DEFINITIONS: include/gd_mesh_clean.h): weld close vertices, drop null
// and duplicate faces, drop small components, repair non-manifold edges and vertices.  fp32 without contraction where the
// header fixes an order; everything else is integers.  One lane per vertex, face, sorted half-edge or corner, 256 per
// workgroup; all of it is bound on gathers.
//
//   check            faces mark used[]; vertices take the exact box: a workgroup combines its order keys with LDS atomics
//                    and sends six device atomics, and one atomicAdd per counter.
//   grid bin         count / scatter of the referenced vertices by integer atomicAdd on the cell; nothing below depends on
//                    the order inside a cell.
//   merge round      Jacobi: reads state_in, writes state_out for every vertex, so a rerun takes the same rounds.
//   edge table       the sorted half-edge keys ARE the table: a run of equal keys is an edge, in ascending face order
//                    (the sort is stable).  Runs are walked, never indexed: no scan and no edge count goes to the host.
//   sweeps           hooking with pointer jumping as in raster_atlas.hip, over consecutive LIVE members of a run.
//   component stats  the open-addressed LDS table of raster_atlas.hip's bounds kernel, with six keys and a count.
//   edge round       one lane per run head walks its run; a nominated face dies by a plain store.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_atlas.h"
#include "../../include/gd_mesh_clean.h"
#include "raster_mesh_common.h"

namespace gd {
namespace {

constexpr int kThreads = 256;
constexpr int kSlots = 64;
constexpr int kProbes = 3;
constexpr uint32_t kKeyMax = 0xFFFFFFFFu;
constexpr int64_t kNoKey = INT64_MAX;
constexpr int kUndecided = 0, kCentre = 1, kMerged = 2;

int cfail(const char* what, const char* msg)
{
    char buf[200];
    snprintf(buf, sizeof(buf), "clean %s: %s", what, msg);
    return mesh_fail(-1, buf);
}

bool faces_ok(int F) { return F >= 1 && F < kMaxFaces; }

bool grid_ok(const gd_remesh_grid* g)
{
    if (!g || !(g->cell > 0.0f) || !isfinite(g->cell)) return false;
    int64_t cells = 1;
    for (int a = 0; a < 3; a++) {
        if (g->dims[a] < 1 || g->dims[a] > GD_MESH_CLEAN_MAX_CELLS || !isfinite(g->origin[a])) return false;
        cells *= g->dims[a];
        if (cells > GD_MESH_CLEAN_MAX_CELLS) return false;
    }
    return true;
}

struct Grid {
    float ox, oy, oz, cell;
    int nx, ny, nz;
};

Grid grid_of_struct(const gd_remesh_grid* g)
{
    return Grid{g->origin[0], g->origin[1], g->origin[2], g->cell, g->dims[0], g->dims[1], g->dims[2]};
}

__device__ __forceinline__ void store_relaxed(int32_t* p, int x)
{
    __hip_atomic_store(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the squared length of the header: each product and each sum rounded on its own
__device__ __forceinline__ float sq3(float x, float y, float z) { return (x * x + y * y) + z * z; }

// One atomicAdd per workgroup: every thread of the workgroup calls this, outside divergent control flow.
__device__ __forceinline__ void block_add(bool mine, int32_t* dst, int* s_count)
{
    if (threadIdx.x == 0) *s_count = 0;
    __syncthreads();
    if (mine) atomicAdd(s_count, 1);
    __syncthreads();
    if (threadIdx.x == 0 && *s_count) atomicAdd(dst, *s_count);
    __syncthreads();
}

// ---- 0 / 1: arguments and box -------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void check_init_kernel(int V, int32_t* __restrict__ used, uint32_t* __restrict__ keys)
{
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v < V) used[v] = 0;
    if (v < 6) keys[v] = v < 3 ? kKeyMax : 0u;
}

__global__ __launch_bounds__(kThreads) void check_faces_kernel(int V, int F, const int32_t* __restrict__ tri, int32_t* used,
                                                               int32_t* stats)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int v = tri[3 * (size_t)f + i];
        if (in_range(v, V)) used[v] = 1;                       // every writer stores the same value
        else atomicOr(&stats[GD_MESH_CLEAN_STAT_INDEX], 1);
    }
}

__global__ __launch_bounds__(kThreads) void check_box_kernel(int V, const float* __restrict__ verts,
                                                             const int32_t* __restrict__ used, uint32_t* keys, int32_t* stats)
{
    __shared__ uint32_t s_key[6];
    __shared__ int s_count;
    if (threadIdx.x < 6) s_key[threadIdx.x] = threadIdx.x < 3 ? kKeyMax : 0u;
    __syncthreads();
    const int v = blockIdx.x * kThreads + threadIdx.x;
    const bool mine = v < V && used[v] != 0;
    bool bad = false;
    if (mine) {
        const V3 p = load3(verts, v);
        bad = !(isfinite(p.x) && isfinite(p.y) && isfinite(p.z));
        if (!bad) {
            atomicMin(&s_key[0], order_key(p.x));
            atomicMin(&s_key[1], order_key(p.y));
            atomicMin(&s_key[2], order_key(p.z));
            atomicMax(&s_key[3], order_key(p.x));
            atomicMax(&s_key[4], order_key(p.y));
            atomicMax(&s_key[5], order_key(p.z));
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&keys[threadIdx.x], s_key[threadIdx.x]);
    else if (threadIdx.x < 6) atomicMax(&keys[threadIdx.x], s_key[threadIdx.x]);
    block_add(mine, &stats[GD_MESH_CLEAN_STAT_REFERENCED], &s_count);
    block_add(bad, &stats[GD_MESH_CLEAN_STAT_NONFINITE], &s_count);
}

__global__ void check_decode_kernel(const uint32_t* __restrict__ keys, float* __restrict__ box)
{
    if (threadIdx.x < 6) box[threadIdx.x] = order_value(keys[threadIdx.x]);
}

// ---- 2: merge -------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int cell_axis(float x, float origin, float cell, int dim)
{
    const float q = floorf((x - origin) / cell);
    return (int)fminf(fmaxf(q, 0.0f), (float)(dim - 1));
}

__device__ __forceinline__ int cell_of(const Grid& g, V3 p)
{
    return (cell_axis(p.z, g.oz, g.cell, g.nz) * g.ny + cell_axis(p.y, g.oy, g.cell, g.ny)) * g.nx +
           cell_axis(p.x, g.ox, g.cell, g.nx);
}

__global__ __launch_bounds__(kThreads) void grid_items_init_kernel(int V, int32_t* __restrict__ items)
{
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v < V) items[v] = -1;
}

__global__ __launch_bounds__(kThreads) void grid_bin_kernel(Grid g, int V, const float* __restrict__ verts,
                                                            const int32_t* __restrict__ used, int scatter, int32_t* count,
                                                            const int32_t* __restrict__ start, int32_t* __restrict__ items)
{
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= V || !used[v]) return;
    const int c = cell_of(g, load3(verts, v));
    const int k = atomicAdd(&count[c], 1);
    if (scatter) {
        const int at = start[c] + k;
        if (in_range(at, V)) items[at] = v;
    }
}

// f(u) for every referenced vertex u in the cells that can hold a vertex close to p, until f returns false
template <typename Fn>
__device__ __forceinline__ void for_each_candidate(const Grid& g, V3 p, int V, const int32_t* __restrict__ start,
                                                   const int32_t* __restrict__ items, Fn f)
{
    const float R = g.cell;
    const int x0 = cell_axis(nextafterf(p.x - R, -INFINITY), g.ox, g.cell, g.nx);
    const int x1 = cell_axis(nextafterf(p.x + R, INFINITY), g.ox, g.cell, g.nx);
    const int y0 = cell_axis(nextafterf(p.y - R, -INFINITY), g.oy, g.cell, g.ny);
    const int y1 = cell_axis(nextafterf(p.y + R, INFINITY), g.oy, g.cell, g.ny);
    const int z0 = cell_axis(nextafterf(p.z - R, -INFINITY), g.oz, g.cell, g.nz);
    const int z1 = cell_axis(nextafterf(p.z + R, INFINITY), g.oz, g.cell, g.nz);
    for (int z = z0; z <= z1; z++)
        for (int y = y0; y <= y1; y++) {
            const int row = (z * g.ny + y) * g.nx;
            // the cells x0 .. x1 of a row are consecutive: one range of items
            const int a = max(start[row + x0], 0), b = min(start[row + x1 + 1], V);
            for (int k = a; k < b; k++) {
                const int u = items[k];
                if (in_range(u, V) && !f(u)) return;
            }
        }
}

__device__ __forceinline__ bool is_close(V3 p, V3 q, float r2)
{
    return sq3(p.x - q.x, p.y - q.y, p.z - q.z) <= r2;
}

__global__ __launch_bounds__(kThreads) void zero_kernel(int n, int32_t* __restrict__ x)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) x[i] = 0;
}

__global__ __launch_bounds__(kThreads) void merge_round_kernel(Grid g, int V, const float* __restrict__ verts,
                                                               const int32_t* __restrict__ used,
                                                               const int32_t* __restrict__ start,
                                                               const int32_t* __restrict__ items, float r2,
                                                               const int32_t* __restrict__ state_in,
                                                               int32_t* __restrict__ state_out, int32_t* undecided)
{
    __shared__ int s_count;
    const int v = blockIdx.x * kThreads + threadIdx.x;
    bool left = false;
    if (v < V) {
        int s = state_in[v];
        if (used[v] && s == kUndecided) {
            const V3 p = load3(verts, v);
            bool centre = false, pending = false;
            for_each_candidate(g, p, V, start, items, [&](int u) {
                if (u >= v || !is_close(p, load3(verts, u), r2)) return true;
                const int su = state_in[u];
                if (su == kCentre) {
                    centre = true;
                    return false;
                }
                pending = pending || su == kUndecided;
                return true;
            });
            s = centre ? kMerged : pending ? kUndecided : kCentre;
            left = s == kUndecided;
        }
        state_out[v] = s;
    }
    block_add(left, undecided, &s_count);
}

__global__ __launch_bounds__(kThreads) void merge_target_kernel(Grid g, int V, const float* __restrict__ verts,
                                                                const int32_t* __restrict__ used,
                                                                const int32_t* __restrict__ start,
                                                                const int32_t* __restrict__ items, float r2, int merge,
                                                                const int32_t* __restrict__ state,
                                                                int32_t* __restrict__ target, int32_t* stats)
{
    __shared__ int s_count;
    const int v = blockIdx.x * kThreads + threadIdx.x;
    bool merged = false;
    if (v < V) {
        int t = -1;
        if (used[v]) {
            t = v;
            if (merge && state[v] != kCentre) {
                const V3 p = load3(verts, v);
                int best = V;
                for_each_candidate(g, p, V, start, items, [&](int u) {
                    if (u < best && state[u] == kCentre && is_close(p, load3(verts, u), r2)) best = u;
                    return true;
                });
                t = best < V ? best : v;
                merged = t != v;
            }
        }
        target[v] = t;
    }
    block_add(merged, &stats[GD_MESH_CLEAN_STAT_MERGED], &s_count);
}

// ---- 3: null faces ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void relabel_kernel(int V, int F, const float* __restrict__ verts,
                                                           const int32_t* __restrict__ tri, const int32_t* __restrict__ target,
                                                           int32_t* __restrict__ tri_out, int32_t* __restrict__ alive,
                                                           float* __restrict__ akey, int32_t* stats)
{
    __shared__ int s_count;
    const int f = blockIdx.x * kThreads + threadIdx.x;
    bool null_face = false;
    if (f < F) {
        int x[3];
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            int v = tri[3 * (size_t)f + i];
            if (in_range(v, V) && target) v = target[v];
            ok = ok && in_range(v, V);
            x[i] = ok ? v : 0;
        }
        float key = 0.0f;
        bool live = ok && x[0] != x[1] && x[1] != x[2] && x[2] != x[0];
        if (live) {
            const V3 n = tri_normal(load3(verts, x[0]), load3(verts, x[1]), load3(verts, x[2]));
            live = isfinite(n.x) && isfinite(n.y) && isfinite(n.z) && (n.x != 0.0f || n.y != 0.0f || n.z != 0.0f);
            if (live) key = sq3(n.x, n.y, n.z);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) tri_out[3 * (size_t)f + i] = x[i];
        alive[f] = live ? 1 : 0;
        akey[f] = key;
        null_face = !live;
    }
    block_add(null_face, &stats[GD_MESH_CLEAN_STAT_NULL], &s_count);
}

// ---- 4: edge table and duplicates -------------------------------------------------------------------------------------

__device__ __forceinline__ int64_t edge_key(int p, int q) { return ((int64_t)min(p, q) << 32) | (int64_t)max(p, q); }

__global__ __launch_bounds__(kThreads) void edge_keys_kernel(int V, int F, const int32_t* __restrict__ tri,
                                                             const int32_t* __restrict__ alive, int64_t* __restrict__ hkeys)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int v[3] = {tri[3 * (size_t)f], tri[3 * (size_t)f + 1], tri[3 * (size_t)f + 2]};
    const bool in = alive[f] && in_range(v[0], V) && in_range(v[1], V) && in_range(v[2], V) && v[0] != v[1] && v[1] != v[2] &&
                    v[2] != v[0];
#pragma unroll
    for (int i = 0; i < 3; i++) hkeys[3 * (size_t)f + i] = in ? edge_key(v[(i + 1) % 3], v[(i + 2) % 3]) : kNoKey;
}

__global__ __launch_bounds__(kThreads) void edge_table_kernel(int n, const int64_t* __restrict__ skeys,
                                                              const int64_t* __restrict__ order, int32_t* __restrict__ she,
                                                              int32_t* __restrict__ pos)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const int64_t h = order[j];
    const bool ok = h >= 0 && h < n;
    she[j] = (ok && skeys[j] != kNoKey) ? (int)h : -1;
    if (ok) pos[h] = j;                                        // order is a permutation: every pos is written once
}

// the vertex of face f that is not on the edge of key k (-1 if f does not hold the edge)
__device__ __forceinline__ int opposite_vertex(const int32_t* __restrict__ tri, int f, int64_t k)
{
    const int a = tri[3 * (size_t)f], b = tri[3 * (size_t)f + 1], c = tri[3 * (size_t)f + 2];
    if (edge_key(b, c) == k) return a;
    if (edge_key(c, a) == k) return b;
    if (edge_key(a, b) == k) return c;
    return -1;
}

__global__ __launch_bounds__(kThreads) void duplicates_kernel(int F, const int32_t* __restrict__ tri,
                                                              const int32_t* __restrict__ alive_in,
                                                              const int64_t* __restrict__ skeys, const int32_t* __restrict__ she,
                                                              const int32_t* __restrict__ pos, int32_t* __restrict__ alive_out,
                                                              int32_t* stats)
{
    __shared__ int s_count;
    const int f = blockIdx.x * kThreads + threadIdx.x;
    bool dup = false;
    if (f < F) {
        const int live = alive_in[f];
        const int a = tri[3 * (size_t)f], b = tri[3 * (size_t)f + 1], c = tri[3 * (size_t)f + 2];
        if (live && a != b && b != c && c != a) {
            const int64_t k0 = edge_key(b, c), k1 = edge_key(c, a), k2 = edge_key(a, b);
            const int i = (k0 <= k1 && k0 <= k2) ? 0 : (k1 <= k2 ? 1 : 2);
            const int64_t k = i == 0 ? k0 : i == 1 ? k1 : k2;
            const int mine = i == 0 ? a : i == 1 ? b : c;
            const int at = pos[3 * (size_t)f + i];
            if (in_range(at, 3 * F) && skeys[at] == k)
                for (int j = at - 1; j >= 0 && skeys[j] == k && !dup; j--) {     // the earlier faces of the run
                    const int h = she[j];
                    if (in_range(h, 3 * F)) dup = opposite_vertex(tri, h / 3, k) == mine;
                }
        }
        alive_out[f] = (live && !dup) ? 1 : 0;
    }
    block_add(dup, &stats[GD_MESH_CLEAN_STAT_DUPLICATE], &s_count);
}

// ---- 5: components ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void iota_kernel(int n, int32_t* __restrict__ x)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) x[i] = i;
}

__device__ __forceinline__ void hook(int32_t* parent, int n, int a, int b, int32_t* changed)
{
    const int ra = root_of(parent, a, n), rb = root_of(parent, b, n);
    if (ra == rb) return;
    atomicMin(parent + max(ra, rb), min(ra, rb));
    store_relaxed(changed, 1);
}

// the half-edge of the previous live face in the run of sorted position j, -1 if there is none
__device__ __forceinline__ int previous_live(const int64_t* __restrict__ skeys, const int32_t* __restrict__ she,
                                             const int32_t* __restrict__ alive, int n, int j)
{
    const int64_t k = skeys[j];
    for (int i = j - 1; i >= 0 && skeys[i] == k; i--) {
        const int h = she[i];
        if (in_range(h, n) && alive[h / 3]) return h;
    }
    return -1;
}

__global__ __launch_bounds__(kThreads) void face_hook_kernel(int F, const int64_t* __restrict__ skeys,
                                                             const int32_t* __restrict__ she, const int32_t* __restrict__ alive,
                                                             int32_t* parent, int32_t* changed)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= 3 * F) return;
    const int h = she[j];
    if (!in_range(h, 3 * F) || !alive[h / 3]) return;
    const int g = previous_live(skeys, she, alive, 3 * F, j);
    if (g >= 0) hook(parent, F, h / 3, g / 3, changed);
}

__global__ __launch_bounds__(kThreads) void jump_kernel(int n, int32_t* parent)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) store_relaxed(parent + i, root_of(parent, i, n));
}

__global__ __launch_bounds__(kThreads) void component_init_kernel(int F, uint32_t* __restrict__ ckeys, int32_t* __restrict__ ccount)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
#pragma unroll
    for (int q = 0; q < 6; q++) ckeys[6 * (size_t)f + q] = q < 3 ? kKeyMax : 0u;
    ccount[f] = 0;
}

__global__ __launch_bounds__(kThreads) void component_stats_kernel(int V, int F, const float* __restrict__ verts,
                                                                   const int32_t* __restrict__ tri,
                                                                   const int32_t* __restrict__ alive,
                                                                   const int32_t* __restrict__ parent, uint32_t* ckeys,
                                                                   int32_t* ccount)
{
    __shared__ int s_label[kSlots];
    __shared__ uint32_t s_key[kSlots][6];
    __shared__ int s_count[kSlots];
    if (threadIdx.x < kSlots) {
        s_label[threadIdx.x] = -1;
        for (int q = 0; q < 6; q++) s_key[threadIdx.x][q] = q < 3 ? kKeyMax : 0u;
        s_count[threadIdx.x] = 0;
    }
    __syncthreads();
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f < F && alive[f]) {
        const int label = parent[f];
        const int x[3] = {tri[3 * (size_t)f], tri[3 * (size_t)f + 1], tri[3 * (size_t)f + 2]};
        if (in_range(label, F) && in_range(x[0], V) && in_range(x[1], V) && in_range(x[2], V)) {
            uint32_t lo[3] = {kKeyMax, kKeyMax, kKeyMax}, hi[3] = {0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const V3 p = load3(verts, x[i]);
                const uint32_t k[3] = {order_key(p.x), order_key(p.y), order_key(p.z)};
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    lo[a] = min(lo[a], k[a]);
                    hi[a] = max(hi[a], k[a]);
                }
            }
            int slot = -1;
            for (int probe = 0; probe < kProbes && slot < 0; probe++) {
                const int s = (label + probe) & (kSlots - 1);
                const int seen = atomicCAS(&s_label[s], -1, label);
                if (seen == -1 || seen == label) slot = s;
            }
            uint32_t* key = slot >= 0 ? s_key[slot] : ckeys + 6 * (size_t)label;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                atomicMin(key + a, lo[a]);
                atomicMax(key + 3 + a, hi[a]);
            }
            atomicAdd(slot >= 0 ? &s_count[slot] : ccount + label, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < kSlots && s_label[threadIdx.x] >= 0) {
        const int label = s_label[threadIdx.x];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            atomicMin(ckeys + 6 * (size_t)label + a, s_key[threadIdx.x][a]);
            atomicMax(ckeys + 6 * (size_t)label + 3 + a, s_key[threadIdx.x][3 + a]);
        }
        atomicAdd(ccount + label, s_count[threadIdx.x]);
    }
}

__global__ __launch_bounds__(kThreads) void component_filter_kernel(int F, const int32_t* __restrict__ alive_in,
                                                                    const int32_t* __restrict__ parent,
                                                                    const uint32_t* __restrict__ ckeys,
                                                                    const int32_t* __restrict__ ccount, int min_faces, float t2,
                                                                    int32_t* __restrict__ label, int32_t* __restrict__ alive_out,
                                                                    int32_t* stats)
{
    __shared__ int s_count;
    const int f = blockIdx.x * kThreads + threadIdx.x;
    bool root = false, removed = false;
    if (f < F) {
        int l = -1, keep = 0;
        if (alive_in[f] && in_range(parent[f], F)) {
            l = parent[f];
            const uint32_t* k = ckeys + 6 * (size_t)l;
            const float ex = order_value(k[3]) - order_value(k[0]), ey = order_value(k[4]) - order_value(k[1]),
                        ez = order_value(k[5]) - order_value(k[2]);
            removed = (min_faces > 0 && ccount[l] < min_faces) || (t2 > 0.0f && sq3(ex, ey, ez) < t2);
            root = l == f;
            keep = removed ? 0 : 1;
        }
        label[f] = l;
        alive_out[f] = keep;
    }
    block_add(root, &stats[GD_MESH_CLEAN_STAT_COMPONENTS], &s_count);
    block_add(root && removed, &stats[GD_MESH_CLEAN_STAT_COMPONENTS_REMOVED], &s_count);
    block_add(removed, &stats[GD_MESH_CLEAN_STAT_COMPONENT_FACES], &s_count);
}

// ---- 6: non-manifold edges ----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void copy_kernel(int n, const int32_t* __restrict__ in, int32_t* __restrict__ out)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) out[i] = in[i];
}

__global__ __launch_bounds__(kThreads) void edge_round_kernel(int F, const int64_t* __restrict__ skeys,
                                                              const int32_t* __restrict__ she, const float* __restrict__ akey,
                                                              const int32_t* __restrict__ live_in, int32_t* live_out,
                                                              int32_t* over)
{
    __shared__ int s_count;
    const int n = 3 * F;
    const int j = blockIdx.x * kThreads + threadIdx.x;
    bool found = false;
    if (j < n) {
        const int64_t k = skeys[j];
        if (k != kNoKey && (j == 0 || skeys[j - 1] != k)) {          // the head of a run walks it
            int count = 0, worst = -1;
            float worst_key = 0.0f;
            for (int i = j; i < n && skeys[i] == k; i++) {
                const int h = she[i];
                if (!in_range(h, n)) continue;
                const int f = h / 3;
                if (!live_in[f]) continue;
                count++;
                const float key = akey[f];
                if (worst < 0 || key < worst_key || (key == worst_key && f > worst)) {
                    worst = f;
                    worst_key = key;
                }
            }
            found = count > 2;
            if (found) live_out[worst] = 0;                            // every writer stores the same value
        }
    }
    block_add(found, over, &s_count);
}

// ---- 7: non-manifold vertices -------------------------------------------------------------------------------------------

__device__ __forceinline__ int corner_of(const int32_t* __restrict__ tri, int f, int v)
{
    if (tri[3 * (size_t)f] == v) return 3 * f;
    if (tri[3 * (size_t)f + 1] == v) return 3 * f + 1;
    if (tri[3 * (size_t)f + 2] == v) return 3 * f + 2;
    return -1;
}

__global__ __launch_bounds__(kThreads) void corner_hook_kernel(int F, const int32_t* __restrict__ tri,
                                                               const int64_t* __restrict__ skeys,
                                                               const int32_t* __restrict__ she,
                                                               const int32_t* __restrict__ alive, int32_t* parent,
                                                               int32_t* changed)
{
    const int n = 3 * F;
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const int h = she[j];
    if (!in_range(h, n) || !alive[h / 3]) return;
    const int g = previous_live(skeys, she, alive, n, j);
    if (g < 0) return;
    const int64_t k = skeys[j];
    const int ends[2] = {(int)(k >> 32), (int)(k & 0xffffffff)};
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int a = corner_of(tri, h / 3, ends[s]), b = corner_of(tri, g / 3, ends[s]);
        if (a >= 0 && b >= 0) hook(parent, n, a, b, changed);
    }
}

__global__ __launch_bounds__(kThreads) void fan_init_kernel(int V, int32_t* __restrict__ vmin, int32_t* __restrict__ used)
{
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v >= V) return;
    if (vmin) vmin[v] = INT32_MAX;
    used[v] = 0;
}

__global__ __launch_bounds__(kThreads) void fan_corners_kernel(int V, int F, const int32_t* __restrict__ tri,
                                                               const int32_t* __restrict__ alive, int32_t* vmin, int32_t* used)
{
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= 3 * F || !alive[c / 3]) return;
    const int v = tri[c];
    if (!in_range(v, V)) return;
    used[v] = 1;
    if (vmin) atomicMin(&vmin[v], c);
}

__global__ __launch_bounds__(kThreads) void fan_keys_kernel(int V, int F, const int32_t* __restrict__ tri,
                                                            const int32_t* __restrict__ alive, const int32_t* __restrict__ parent,
                                                            const int32_t* __restrict__ vmin, int64_t* __restrict__ split_key,
                                                            int32_t* stats)
{
    __shared__ int s_count;
    const int c = blockIdx.x * kThreads + threadIdx.x;
    bool split = false;
    if (c < 3 * F) {
        int64_t key = kNoKey;
        const int v = tri[c];
        if (alive[c / 3] && in_range(v, V) && parent[c] == c && vmin[v] != c) {
            // the fan of vmin[v] has vmin[v] as its root: a root that is not vmin[v] is another fan
            key = ((int64_t)v << 32) | (int64_t)c;
            split = true;
        }
        split_key[c] = key;
    }
    block_add(split, &stats[GD_MESH_CLEAN_STAT_SPLIT], &s_count);
}

__global__ __launch_bounds__(kThreads) void fill_kernel(int n, int32_t value, int32_t* __restrict__ x)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) x[i] = value;
}

__global__ __launch_bounds__(kThreads) void fan_ranks_kernel(int n, int S, const int64_t* __restrict__ sorted_keys,
                                                             int32_t* __restrict__ crank)
{
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= S) return;
    const int c = (int)(sorted_keys[k] & 0xffffffff);
    if (in_range(c, n)) crank[c] = k;
}

// ---- 8: output ------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void emit_faces_kernel(int V, int F, int Fout, int V0, int S,
                                                              const int32_t* __restrict__ tri, const int32_t* __restrict__ alive,
                                                              const int32_t* __restrict__ fscan, const int32_t* __restrict__ vscan,
                                                              const int32_t* __restrict__ parent, const int32_t* __restrict__ crank,
                                                              int32_t* __restrict__ tri_out, int32_t* __restrict__ face_map)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F || !alive[f]) return;
    const int at = fscan[f];
    if (!in_range(at, Fout)) return;
    face_map[at] = f;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int c = 3 * f + i, v = tri[c];
        int row = in_range(v, V) ? vscan[v] : 0;
        if (S > 0) {
            const int root = parent[c];
            const int rank = in_range(root, 3 * F) ? crank[root] : -1;
            if (in_range(rank, S)) row = V0 + rank;
        }
        tri_out[3 * (size_t)at + i] = in_range(row, V0 + S) ? row : 0;
    }
}

__global__ __launch_bounds__(kThreads) void emit_vertices_kernel(int V, int V0, int S, const float* __restrict__ verts,
                                                                 const int32_t* __restrict__ used,
                                                                 const int32_t* __restrict__ vscan,
                                                                 const int32_t* __restrict__ target,
                                                                 const int64_t* __restrict__ sorted_keys,
                                                                 float* __restrict__ verts_out, int32_t* __restrict__ vertex_map)
{
    const int v = blockIdx.x * kThreads + threadIdx.x;
    if (v < V) {
        if (used[v] && in_range(vscan[v], V0)) store3(verts_out, vscan[v], load3(verts, v));
        const int t = target ? target[v] : v;
        vertex_map[v] = (in_range(t, V) && used[t] && in_range(vscan[t], V0)) ? vscan[t] : -1;
    }
    if (v < S) {
        const int src = (int)(sorted_keys[v] >> 32);
        store3(verts_out, (size_t)V0 + v, in_range(src, V) ? load3(verts, src) : V3{0.0f, 0.0f, 0.0f});
    }
}

__global__ __launch_bounds__(kThreads) void compact_faces_kernel(int F, int Fout, const int32_t* __restrict__ tri,
                                                                 const int32_t* __restrict__ alive,
                                                                 const int32_t* __restrict__ fscan, int32_t* __restrict__ tri_out,
                                                                 int32_t* __restrict__ face_map)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F || !alive[f]) return;
    const int at = fscan[f];
    if (!in_range(at, Fout)) return;
    face_map[at] = f;
#pragma unroll
    for (int i = 0; i < 3; i++) tri_out[3 * (size_t)at + i] = tri[3 * (size_t)f + i];
}

bool rounds_ok(int rounds, bool even) { return rounds >= 1 && rounds <= GD_MESH_CLEAN_MAX_ROUNDS && !(even && rounds % 2); }

}  // namespace
}  // namespace gd

extern "C" {

using namespace gd;

int gd_mesh_clean_check(void* stream, int V, int F, const float* verts, const int32_t* tri, int32_t* used, float* box,
                        uint32_t* box_keys, int32_t* stats)
{
    const char* what = "check";
    if (!verts || !tri || !used || !box || !box_keys || !stats) return cfail(what, "null pointer");
    if (V < 1 || !faces_ok(F)) return cfail(what, "V must be at least 1 and F in 1..2^29-1");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(check_init_kernel, grid_of(max(V, 6)), dim3(kThreads), 0, s, V, used, box_keys);
    hipLaunchKernelGGL(check_faces_kernel, grid_of(F), dim3(kThreads), 0, s, V, F, tri, used, stats);
    hipLaunchKernelGGL(check_box_kernel, grid_of(V), dim3(kThreads), 0, s, V, verts, used, box_keys, stats);
    hipLaunchKernelGGL(check_decode_kernel, dim3(1), dim3(64), 0, s, box_keys, box);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_grid_bin(void* stream, const gd_remesh_grid* grid, int V, const float* verts, const int32_t* used,
                           int scatter, int32_t* count, const int32_t* start, int32_t* items)
{
    const char* what = "grid bin";
    if (!grid_ok(grid)) return cfail(what, "the grid needs a positive finite cell and 1..2^21 cells");
    if (!verts || !used || !count || (scatter && (!start || !items))) return cfail(what, "null pointer");
    if (V < 1) return cfail(what, "V must be at least 1");
    hipStream_t s = (hipStream_t)stream;
    if (scatter) hipLaunchKernelGGL(grid_items_init_kernel, grid_of(V), dim3(kThreads), 0, s, V, items);
    hipLaunchKernelGGL(grid_bin_kernel, grid_of(V), dim3(kThreads), 0, s, grid_of_struct(grid), V, verts, used, scatter, count,
                       start, items);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_merge_rounds(void* stream, const gd_remesh_grid* grid, int V, const float* verts, const int32_t* used,
                               const int32_t* start, const int32_t* items, float r2, int rounds, int32_t* state_a,
                               int32_t* state_b, int32_t* undecided)
{
    const char* what = "merge rounds";
    if (!grid_ok(grid)) return cfail(what, "the grid needs a positive finite cell and 1..2^21 cells");
    if (!verts || !used || !start || !items || !state_a || !state_b || !undecided) return cfail(what, "null pointer");
    if (state_a == state_b) return cfail(what, "state_a and state_b must be distinct buffers");
    if (V < 1 || !(r2 >= 0.0f) || !isfinite(r2)) return cfail(what, "V must be at least 1 and r2 finite and >= 0");
    if (!rounds_ok(rounds, true)) return cfail(what, "rounds must be even and in 2..16");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(zero_kernel, grid_of(rounds), dim3(kThreads), 0, s, rounds, undecided);
    for (int k = 0; k < rounds; k++)
        hipLaunchKernelGGL(merge_round_kernel, grid_of(V), dim3(kThreads), 0, s, grid_of_struct(grid), V, verts, used, start,
                           items, r2, k % 2 ? state_b : state_a, k % 2 ? state_a : state_b, undecided + k);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_merge_target(void* stream, const gd_remesh_grid* grid, int V, const float* verts, const int32_t* used,
                               const int32_t* start, const int32_t* items, float r2, int merge, const int32_t* state,
                               int32_t* target, int32_t* stats)
{
    const char* what = "merge target";
    if (merge && !grid_ok(grid)) return cfail(what, "the grid needs a positive finite cell and 1..2^21 cells");
    if (!verts || !used || !target || !stats || (merge && (!start || !items || !state))) return cfail(what, "null pointer");
    if (V < 1 || (merge && (!(r2 >= 0.0f) || !isfinite(r2)))) return cfail(what, "V must be at least 1 and r2 finite and >= 0");
    hipLaunchKernelGGL(merge_target_kernel, grid_of(V), dim3(kThreads), 0, (hipStream_t)stream,
                       merge ? grid_of_struct(grid) : Grid{0, 0, 0, 1, 1, 1, 1}, V, verts, used, start, items, r2, merge, state,
                       target, stats);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_relabel(void* stream, int V, int F, const float* verts, const int32_t* tri, const int32_t* target,
                          int32_t* tri_out, int32_t* alive, float* akey, int32_t* stats)
{
    const char* what = "relabel";
    if (!verts || !tri || !tri_out || !alive || !akey || !stats) return cfail(what, "null pointer");
    if (V < 1 || !faces_ok(F)) return cfail(what, "V must be at least 1 and F in 1..2^29-1");
    hipLaunchKernelGGL(relabel_kernel, grid_of(F), dim3(kThreads), 0, (hipStream_t)stream, V, F, verts, tri, target, tri_out,
                       alive, akey, stats);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_edge_keys(void* stream, int V, int F, const int32_t* tri, const int32_t* alive, int64_t* hkeys)
{
    const char* what = "edge keys";
    if (!tri || !alive || !hkeys) return cfail(what, "null pointer");
    if (V < 1 || !faces_ok(F)) return cfail(what, "V must be at least 1 and F in 1..2^29-1");
    hipLaunchKernelGGL(edge_keys_kernel, grid_of(F), dim3(kThreads), 0, (hipStream_t)stream, V, F, tri, alive, hkeys);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_edge_table(void* stream, int n, const int64_t* skeys, const int64_t* order, int32_t* she, int32_t* pos)
{
    const char* what = "edge table";
    if (!skeys || !order || !she || !pos) return cfail(what, "null pointer");
    if (n < 3 || n % 3 || !faces_ok(n / 3)) return cfail(what, "n must be 3F with F in 1..2^29-1");
    hipLaunchKernelGGL(edge_table_kernel, grid_of(n), dim3(kThreads), 0, (hipStream_t)stream, n, skeys, order, she, pos);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_duplicates(void* stream, int F, const int32_t* tri, const int32_t* alive_in, const int64_t* skeys,
                             const int32_t* she, const int32_t* pos, int32_t* alive_out, int32_t* stats)
{
    const char* what = "duplicates";
    if (!tri || !alive_in || !skeys || !she || !pos || !alive_out || !stats) return cfail(what, "null pointer");
    if (alive_in == alive_out) return cfail(what, "alive_in and alive_out must be distinct buffers");
    if (!faces_ok(F)) return cfail(what, "F must be in 1..2^29-1");
    hipLaunchKernelGGL(duplicates_kernel, grid_of(F), dim3(kThreads), 0, (hipStream_t)stream, F, tri, alive_in, skeys, she, pos,
                       alive_out, stats);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_face_sweeps(void* stream, int F, const int64_t* skeys, const int32_t* she, const int32_t* alive,
                              int sweeps, int init, int32_t* parent, int32_t* changed)
{
    const char* what = "face sweeps";
    if (!skeys || !she || !alive || !parent || !changed) return cfail(what, "null pointer");
    if (!faces_ok(F)) return cfail(what, "F must be in 1..2^29-1");
    if (!rounds_ok(sweeps, false)) return cfail(what, "sweeps must be in 1..16");
    hipStream_t s = (hipStream_t)stream;
    if (init) hipLaunchKernelGGL(iota_kernel, grid_of(F), dim3(kThreads), 0, s, F, parent);
    hipLaunchKernelGGL(zero_kernel, grid_of(sweeps), dim3(kThreads), 0, s, sweeps, changed);
    for (int k = 0; k < sweeps; k++) {
        hipLaunchKernelGGL(face_hook_kernel, grid_of(3 * F), dim3(kThreads), 0, s, F, skeys, she, alive, parent, changed + k);
        hipLaunchKernelGGL(jump_kernel, grid_of(F), dim3(kThreads), 0, s, F, parent);
    }
    return mesh_launched("clean", what);
}

int gd_mesh_clean_component_stats(void* stream, int V, int F, const float* verts, const int32_t* tri, const int32_t* alive,
                                  const int32_t* parent, uint32_t* ckeys, int32_t* ccount)
{
    const char* what = "component stats";
    if (!verts || !tri || !alive || !parent || !ckeys || !ccount) return cfail(what, "null pointer");
    if (V < 1 || !faces_ok(F)) return cfail(what, "V must be at least 1 and F in 1..2^29-1");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(component_init_kernel, grid_of(F), dim3(kThreads), 0, s, F, ckeys, ccount);
    hipLaunchKernelGGL(component_stats_kernel, grid_of(F), dim3(kThreads), 0, s, V, F, verts, tri, alive, parent, ckeys, ccount);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_component_filter(void* stream, int F, const int32_t* alive_in, const int32_t* parent,
                                   const uint32_t* ckeys, const int32_t* ccount, int min_faces, float t2, int32_t* label,
                                   int32_t* alive_out, int32_t* stats)
{
    const char* what = "component filter";
    if (!alive_in || !parent || !ckeys || !ccount || !label || !alive_out || !stats) return cfail(what, "null pointer");
    if (alive_in == alive_out) return cfail(what, "alive_in and alive_out must be distinct buffers");
    if (!faces_ok(F)) return cfail(what, "F must be in 1..2^29-1");
    if (!(t2 >= 0.0f)) return cfail(what, "t2 must be >= 0");
    hipLaunchKernelGGL(component_filter_kernel, grid_of(F), dim3(kThreads), 0, (hipStream_t)stream, F, alive_in, parent, ckeys,
                       ccount, min_faces, t2, label, alive_out, stats);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_edge_rounds(void* stream, int F, const int64_t* skeys, const int32_t* she, const float* akey, int rounds,
                              int32_t* live_a, int32_t* live_b, int32_t* over)
{
    const char* what = "edge rounds";
    if (!skeys || !she || !akey || !live_a || !live_b || !over) return cfail(what, "null pointer");
    if (live_a == live_b) return cfail(what, "live_a and live_b must be distinct buffers");
    if (!faces_ok(F)) return cfail(what, "F must be in 1..2^29-1");
    if (!rounds_ok(rounds, true)) return cfail(what, "rounds must be even and in 2..16");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(zero_kernel, grid_of(rounds), dim3(kThreads), 0, s, rounds, over);
    for (int k = 0; k < rounds; k++) {
        int32_t* in = k % 2 ? live_b : live_a;
        int32_t* out = k % 2 ? live_a : live_b;
        hipLaunchKernelGGL(copy_kernel, grid_of(F), dim3(kThreads), 0, s, F, in, out);
        hipLaunchKernelGGL(edge_round_kernel, grid_of(3 * F), dim3(kThreads), 0, s, F, skeys, she, akey, in, out, over + k);
    }
    return mesh_launched("clean", what);
}

int gd_mesh_clean_corner_sweeps(void* stream, int F, const int32_t* tri, const int64_t* skeys, const int32_t* she,
                                const int32_t* alive, int sweeps, int init, int32_t* parent, int32_t* changed)
{
    const char* what = "corner sweeps";
    if (!tri || !skeys || !she || !alive || !parent || !changed) return cfail(what, "null pointer");
    if (!faces_ok(F)) return cfail(what, "F must be in 1..2^29-1");
    if (!rounds_ok(sweeps, false)) return cfail(what, "sweeps must be in 1..16");
    hipStream_t s = (hipStream_t)stream;
    if (init) hipLaunchKernelGGL(iota_kernel, grid_of(3 * F), dim3(kThreads), 0, s, 3 * F, parent);
    hipLaunchKernelGGL(zero_kernel, grid_of(sweeps), dim3(kThreads), 0, s, sweeps, changed);
    for (int k = 0; k < sweeps; k++) {
        hipLaunchKernelGGL(corner_hook_kernel, grid_of(3 * F), dim3(kThreads), 0, s, F, tri, skeys, she, alive, parent,
                           changed + k);
        hipLaunchKernelGGL(jump_kernel, grid_of(3 * F), dim3(kThreads), 0, s, 3 * F, parent);
    }
    return mesh_launched("clean", what);
}

int gd_mesh_clean_fan_roots(void* stream, int V, int F, const int32_t* tri, const int32_t* alive, const int32_t* parent,
                            int32_t* vmin, int32_t* used, int64_t* split_key, int32_t* stats)
{
    const char* what = "fan roots";
    if (!tri || !alive || !used || !stats || (parent && (!vmin || !split_key))) return cfail(what, "null pointer");
    if (V < 1 || !faces_ok(F)) return cfail(what, "V must be at least 1 and F in 1..2^29-1");
    hipStream_t s = (hipStream_t)stream;
    int32_t* lowest = parent ? vmin : nullptr;
    hipLaunchKernelGGL(fan_init_kernel, grid_of(V), dim3(kThreads), 0, s, V, lowest, used);
    hipLaunchKernelGGL(fan_corners_kernel, grid_of(3 * F), dim3(kThreads), 0, s, V, F, tri, alive, lowest, used);
    if (parent)
        hipLaunchKernelGGL(fan_keys_kernel, grid_of(3 * F), dim3(kThreads), 0, s, V, F, tri, alive, parent, vmin, split_key, stats);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_fan_ranks(void* stream, int n, int S, const int64_t* sorted_keys, int32_t* crank)
{
    const char* what = "fan ranks";
    if (!sorted_keys || !crank) return cfail(what, "null pointer");
    if (n < 3 || n % 3 || !faces_ok(n / 3) || S < 0 || S > n) return cfail(what, "n must be 3F with F in 1..2^29-1 and S in 0..n");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fill_kernel, grid_of(n), dim3(kThreads), 0, s, n, -1, crank);
    if (S > 0) hipLaunchKernelGGL(fan_ranks_kernel, grid_of(S), dim3(kThreads), 0, s, n, S, sorted_keys, crank);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_compact_faces(void* stream, int F, int Fout, const int32_t* tri, const int32_t* alive,
                                const int32_t* fscan, int32_t* tri_out, int32_t* face_map)
{
    const char* what = "compact faces";
    if (!tri || !alive || !fscan || !tri_out || !face_map) return cfail(what, "null pointer");
    if (!faces_ok(F) || Fout < 1 || Fout > F) return cfail(what, "F must be in 1..2^29-1 and Fout in 1..F");
    hipLaunchKernelGGL(compact_faces_kernel, grid_of(F), dim3(kThreads), 0, (hipStream_t)stream, F, Fout, tri, alive, fscan,
                       tri_out, face_map);
    return mesh_launched("clean", what);
}

int gd_mesh_clean_emit(void* stream, int V, int F, int Fout, int V0, int S, const float* verts, const int32_t* tri,
                       const int32_t* alive, const int32_t* fscan, const int32_t* used, const int32_t* vscan,
                       const int32_t* target, const int32_t* parent, const int32_t* crank, const int64_t* sorted_keys,
                       float* verts_out, int32_t* tri_out, int32_t* face_map, int32_t* vertex_map)
{
    const char* what = "emit";
    if (!verts || !tri || !alive || !fscan || !used || !vscan || !verts_out || !tri_out || !face_map || !vertex_map)
        return cfail(what, "null pointer");
    if (V < 1 || !faces_ok(F) || Fout < 1 || Fout > F || V0 < 1 || V0 > V || S < 0 || (int64_t)S > 3 * (int64_t)Fout ||
        (int64_t)V0 + S >= (int64_t)1 << 31)
        return cfail(what, "V >= 1, F in 1..2^29-1, Fout in 1..F, V0 in 1..V, S in 0..3 Fout, V0 + S < 2^31");
    if (S > 0 && (!parent || !crank || !sorted_keys)) return cfail(what, "S > 0 needs parent, crank and sorted_keys");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(emit_faces_kernel, grid_of(F), dim3(kThreads), 0, s, V, F, Fout, V0, S, tri, alive, fscan, vscan, parent,
                       crank, tri_out, face_map);
    hipLaunchKernelGGL(emit_vertices_kernel, grid_of(max(V, S)), dim3(kThreads), 0, s, V, V0, S, verts, used, vscan, target,
                       sorted_keys, verts_out, vertex_map);
    return mesh_launched("clean", what);
}

}  // extern "C"
