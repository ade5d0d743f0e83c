// raster_atlas.hip -- the chart-based UV atlas of the textured-mesh export (C-ABI and the DEFINITIONS: include/gd_atlas.h):
// face classes, charts as connected components, per-chart bounds, corner coordinates, welded vt rows and the lost faces of
// the overlap peeling.  fp32 without contraction where the header fixes an order; everything else is integers.
//
//   face class   one thread per face.
//   hook         one thread per edge: follows parent to the two roots (parent[x] <= x, so the walk ends) and hooks the
//                higher root under the lower with a 32-bit atomicMin; any hook raises the sweep's changed flag.
//   jump         one thread per face: parent[f] = its root.  Plain stores race only with loads that would read either
//                the old or the new value, and both are members of the component on the way to the root.
//   bounds       one workgroup of 256 faces.  Consecutive faces mostly share a handful of charts, so the workgroup keeps
//                an open-addressed LDS table of kSlots charts (claimed by atomicCAS on the chart id, three probes) with
//                the four order-preserving keys and the face count; LDS atomics combine, then one thread per used slot
//                sends five device-scope atomics to memory.  A face that finds no slot goes to memory directly.
//   emit         one thread per corner.
//   write vt     one thread per corner: corners of one row hold equal values, so the stores do not race in value.
//   lost faces   one wave per face, four faces per workgroup: the lanes stride over the texels of the face's bounding
//                box with the int64 edge functions of the rasterizer; __any ends the walk at the first foreign owner.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_atlas.h"
#include "raster_mesh_common.h"

namespace gd {
namespace {

constexpr int kThreads = 256;
constexpr int kSlots = 64;
constexpr int kProbes = 3;
constexpr uint32_t kKeyMax = 0xFFFFFFFFu;

int afail(const char* what, const char* msg)
{
    char buf[200];
    snprintf(buf, sizeof(buf), "atlas %s: %s", what, msg);
    return mesh_fail(-1, buf);
}

// the corner's (a, b) of the header for a class 0..5
__device__ __forceinline__ void project(int cls, const float* p, float& a, float& b)
{
    const int k = cls >> 1, k1 = k == 2 ? 0 : k + 1, k2 = k1 == 2 ? 0 : k1 + 1;
    a = (cls & 1) ? p[k2] : p[k1];
    b = (cls & 1) ? p[k1] : p[k2];
}

__global__ __launch_bounds__(kThreads) void face_class_kernel(int V, int F, const float* __restrict__ verts,
                                                              const int32_t* __restrict__ tri, int32_t* __restrict__ cls)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int i0 = tri[3 * (size_t)f], i1 = tri[3 * (size_t)f + 1], i2 = tri[3 * (size_t)f + 2];
    int out = GD_ATLAS_DEGENERATE;
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
        const float* p0 = verts + 3 * (size_t)i0;
        const float* p1 = verts + 3 * (size_t)i1;
        const float* p2 = verts + 3 * (size_t)i2;
        const float ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
        const float wx = p2[0] - p0[0], wy = p2[1] - p0[1], wz = p2[2] - p0[2];
        const float n[3] = {uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx};
        const bool finite = isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]);
        if (finite && (n[0] != 0.0f || n[1] != 0.0f || n[2] != 0.0f)) {
            int k = 0;
            if (fabsf(n[1]) > fabsf(n[k])) k = 1;
            if (fabsf(n[2]) > fabsf(n[k])) k = 2;
            out = 2 * k + (n[k] < 0.0f ? 1 : 0);
        }
    }
    cls[f] = out;
}

__global__ __launch_bounds__(kThreads) void hook_kernel(int F, int E, const int32_t* __restrict__ eh,
                                                        const int32_t* __restrict__ cls, const int32_t* __restrict__ layer,
                                                        const int32_t* __restrict__ single, int32_t* parent, int32_t* changed)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= E) return;
    const int h0 = eh[2 * (size_t)e], h1 = eh[2 * (size_t)e + 1];
    if (h0 < 0 || h1 < 0) return;
    const int f = h0 / 3, g = h1 / 3;
    if (f >= F || g >= F || f == g) return;
    const int c = cls[f];
    if (c != cls[g] || c < 0 || c >= GD_ATLAS_DEGENERATE || layer[f] != layer[g] || single[f] || single[g]) return;
    const int rf = root_of(parent, f, F), rg = root_of(parent, g, F);
    if (rf == rg) return;
    atomicMin(parent + (rf > rg ? rf : rg), rf < rg ? rf : rg);
    __hip_atomic_store(changed, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void jump_kernel(int F, int32_t* parent)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    const int r = root_of(parent, f, F);
    __hip_atomic_store(parent + f, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kThreads) void roots_kernel(int F, const int32_t* __restrict__ cls,
                                                         const int32_t* __restrict__ parent, int32_t* __restrict__ is_root)
{
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= F) return;
    is_root[f] = (parent[f] == f && cls[f] != GD_ATLAS_DEGENERATE) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void bounds_init_kernel(int C, uint32_t* __restrict__ keys, int32_t* __restrict__ count)
{
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    keys[4 * (size_t)c] = kKeyMax;
    keys[4 * (size_t)c + 1] = kKeyMax;
    keys[4 * (size_t)c + 2] = 0u;
    keys[4 * (size_t)c + 3] = 0u;
    count[c] = 0;
}

__global__ __launch_bounds__(kThreads) void bounds_kernel(int V, int F, int C, const float* __restrict__ verts,
                                                          const int32_t* __restrict__ tri, const int32_t* __restrict__ cls,
                                                          const int32_t* __restrict__ parent, const int32_t* __restrict__ scan,
                                                          int32_t* __restrict__ face_chart, uint32_t* keys, int32_t* count)
{
    __shared__ int s_chart[kSlots];
    __shared__ uint32_t s_key[kSlots][4];
    __shared__ int s_count[kSlots];
    if (threadIdx.x < kSlots) {
        s_chart[threadIdx.x] = -1;
        s_key[threadIdx.x][0] = kKeyMax;
        s_key[threadIdx.x][1] = kKeyMax;
        s_key[threadIdx.x][2] = 0u;
        s_key[threadIdx.x][3] = 0u;
        s_count[threadIdx.x] = 0;
    }
    __syncthreads();
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f < F) {
        const int c6 = cls[f], label = parent[f];
        int chart = -1;
        if (c6 >= 0 && c6 < GD_ATLAS_DEGENERATE && label >= 0 && label < F) {
            chart = scan[label];
            if (chart < 0 || chart >= C) chart = -1;
        }
        const int i0 = tri[3 * (size_t)f], i1 = tri[3 * (size_t)f + 1], i2 = tri[3 * (size_t)f + 2];
        if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) chart = -1;
        face_chart[f] = chart;
        if (chart >= 0) {
            uint32_t lo_a = kKeyMax, lo_b = kKeyMax, hi_a = 0u, hi_b = 0u;
            const int idx[3] = {i0, i1, i2};
            for (int i = 0; i < 3; i++) {
                float a, b;
                project(c6, verts + 3 * (size_t)idx[i], a, b);
                const uint32_t ka = order_key(a), kb = order_key(b);
                lo_a = min(lo_a, ka);
                hi_a = max(hi_a, ka);
                lo_b = min(lo_b, kb);
                hi_b = max(hi_b, kb);
            }
            int slot = -1;
            for (int probe = 0; probe < kProbes && slot < 0; probe++) {
                const int s = (chart + probe) & (kSlots - 1);
                const int seen = atomicCAS(&s_chart[s], -1, chart);
                if (seen == -1 || seen == chart) slot = s;
            }
            if (slot >= 0) {
                atomicMin(&s_key[slot][0], lo_a);
                atomicMin(&s_key[slot][1], lo_b);
                atomicMax(&s_key[slot][2], hi_a);
                atomicMax(&s_key[slot][3], hi_b);
                atomicAdd(&s_count[slot], 1);
            } else {
                atomicMin(keys + 4 * (size_t)chart, lo_a);
                atomicMin(keys + 4 * (size_t)chart + 1, lo_b);
                atomicMax(keys + 4 * (size_t)chart + 2, hi_a);
                atomicMax(keys + 4 * (size_t)chart + 3, hi_b);
                atomicAdd(count + chart, 1);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < kSlots && s_chart[threadIdx.x] >= 0) {
        const int chart = s_chart[threadIdx.x];
        atomicMin(keys + 4 * (size_t)chart, s_key[threadIdx.x][0]);
        atomicMin(keys + 4 * (size_t)chart + 1, s_key[threadIdx.x][1]);
        atomicMax(keys + 4 * (size_t)chart + 2, s_key[threadIdx.x][2]);
        atomicMax(keys + 4 * (size_t)chart + 3, s_key[threadIdx.x][3]);
        atomicAdd(count + chart, s_count[threadIdx.x]);
    }
}

__global__ __launch_bounds__(kThreads) void bounds_decode_kernel(int n, const uint32_t* __restrict__ keys,
                                                                 float* __restrict__ bounds)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n) bounds[i] = order_value(keys[i]);
}

__global__ __launch_bounds__(kThreads) void emit_kernel(int V, int F, int C, int gutter, float scale,
                                                        const float* __restrict__ verts, const int32_t* __restrict__ tri,
                                                        const int32_t* __restrict__ cls, const int32_t* __restrict__ face_chart,
                                                        const float* __restrict__ bounds, const int32_t* __restrict__ offsets,
                                                        int32_t* __restrict__ corner_xy, int64_t* __restrict__ key)
{
    const int64_t corner = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (corner >= 3 * (int64_t)F) return;
    const int f = (int)(corner / 3);
    const int chart = face_chart[f], c6 = cls[f], v = tri[corner];
    int X = 0, Y = 0;
    int64_t k = (int64_t)C << 32;
    if (chart >= 0 && chart < C && c6 >= 0 && c6 < GD_ATLAS_DEGENERATE && v >= 0 && v < V) {
        float a, b;
        project(c6, verts + 3 * (size_t)v, a, b);
        const float a_min = bounds[4 * (size_t)chart], b_min = bounds[4 * (size_t)chart + 1];
        const float da = ((a - a_min) * scale) * 256.0f, db = ((b - b_min) * scale) * 256.0f;
        X = 256 * (offsets[2 * (size_t)chart] + gutter) + (int)rintf(da);
        Y = 256 * (offsets[2 * (size_t)chart + 1] + gutter) + (int)rintf(db);
        k = ((int64_t)chart << 32) | (int64_t)v;
    }
    corner_xy[2 * corner] = X;
    corner_xy[2 * corner + 1] = Y;
    key[corner] = k;
}

__global__ __launch_bounds__(kThreads) void write_vt_kernel(int n, int T, float denom, const int64_t* __restrict__ row,
                                                            const int32_t* __restrict__ corner_xy, float* vt,
                                                            int32_t* __restrict__ ft)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t r = row[i];
    const bool ok = r >= 0 && r < T;
    ft[i] = ok ? (int32_t)r : 0;
    if (!ok) return;
    vt[2 * r] = (float)corner_xy[2 * (size_t)i] / denom;
    vt[2 * r + 1] = (float)corner_xy[2 * (size_t)i + 1] / denom;
}

// an edge function's verdict at one centre, by the rule of gd_mesh.h
__device__ __forceinline__ bool edge_in(int64_t e, int64_t dX, int64_t dY)
{
    return e > 0 || (e == 0 && (dY > 0 || (dY == 0 && dX < 0)));
}

constexpr int kLostWaves = kThreads / 64;

__global__ __launch_bounds__(kThreads) void lost_faces_kernel(int F, int H, int W, const int32_t* __restrict__ corner_xy,
                                                              const float* __restrict__ rast, int freeze,
                                                              int32_t* __restrict__ lost, int32_t* __restrict__ layer,
                                                              int32_t* __restrict__ single)
{
    const int lane = threadIdx.x & 63;
    const int f = blockIdx.x * kLostWaves + (threadIdx.x >> 6);   // wave-uniform
    if (f >= F) return;
    int64_t X[3], Y[3];
    for (int i = 0; i < 3; i++) {
        X[i] = corner_xy[6 * (size_t)f + 2 * i];
        Y[i] = corner_xy[6 * (size_t)f + 2 * i + 1];
    }
    const int64_t A = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0]);
    bool is_lost = false;
    if (A != 0) {
        const int64_t sign = A > 0 ? 1 : -1;
        const int64_t x_lo = min(X[0], min(X[1], X[2])), x_hi = max(X[0], max(X[1], X[2]));
        const int64_t y_lo = min(Y[0], min(Y[1], Y[2])), y_hi = max(Y[0], max(Y[1], Y[2]));
        // centres 256 c + 128 inside [lo, hi]: ceil((lo - 128) / 256) .. floor((hi - 128) / 256), arithmetic shifts
        const int c0 = (int)max((int64_t)0, (x_lo - 128 + 255) >> 8), c1 = (int)min((int64_t)W - 1, (x_hi - 128) >> 8);
        const int r0 = (int)max((int64_t)0, (y_lo - 128 + 255) >> 8), r1 = (int)min((int64_t)H - 1, (y_hi - 128) >> 8);
        if (c1 >= c0 && r1 >= r0) {
            const int bw = c1 - c0 + 1;
            const int64_t cells = (int64_t)bw * (r1 - r0 + 1);
            for (int64_t base = 0; base < cells; base += 64) {                 // wave-uniform trip count
                const int64_t cell = base + lane;
                bool foreign = false;
                if (cell < cells) {
                    const int r = r0 + (int)(cell / bw), c = c0 + (int)(cell % bw);
                    const int64_t Px = 256 * (int64_t)c + 128, Py = 256 * (int64_t)r + 128;
                    bool inside = true;
                    for (int i = 0; i < 3; i++) {
                        const int j = i == 2 ? 0 : i + 1, k = j == 2 ? 0 : j + 1;
                        const int64_t dX = sign * (X[k] - X[j]), dY = sign * (Y[k] - Y[j]);
                        inside = inside && edge_in(dX * (Py - Y[j]) - dY * (Px - X[j]), dX, dY);
                    }
                    if (inside) foreign = (int)rast[4 * ((size_t)r * W + c) + 3] - 1 != f;
                }
                if (__any(foreign)) {
                    is_lost = true;
                    break;
                }
            }
        }
    }
    if (lane == 0) {
        lost[f] = is_lost ? 1 : 0;
        if (is_lost) {
            if (freeze) single[f] = 1;
            else layer[f] += 1;
        }
    }
}

bool faces_ok(int F) { return F >= 1 && F < kMaxFaces; }

}  // namespace
}  // namespace gd

extern "C" {

using namespace gd;

int gd_atlas_face_class(void* stream, int V, int F, const float* verts, const int32_t* tri, int32_t* cls)
{
    const char* what = "face class";
    if (!verts || !tri || !cls) return afail(what, "null pointer");
    if (V < 1 || !faces_ok(F)) return afail(what, "V must be at least 1 and F in 1..2^29-1");
    hipLaunchKernelGGL(face_class_kernel, grid_of(F), dim3(kThreads), 0, (hipStream_t)stream, V, F, verts, tri, cls);
    return mesh_launched("atlas", what);
}

int gd_atlas_hook(void* stream, int F, int E, const int32_t* eh, const int32_t* cls, const int32_t* layer,
                  const int32_t* single, int32_t* parent, int32_t* changed)
{
    const char* what = "hook";
    if (!eh || !cls || !layer || !single || !parent || !changed) return afail(what, "null pointer");
    if (!faces_ok(F) || E < 1 || (int64_t)E > 3 * (int64_t)F) return afail(what, "F must be in 1..2^29-1 and E in 1..3F");
    hipLaunchKernelGGL(hook_kernel, grid_of(E), dim3(kThreads), 0, (hipStream_t)stream, F, E, eh, cls, layer, single, parent,
                       changed);
    return mesh_launched("atlas", what);
}

int gd_atlas_jump(void* stream, int F, int32_t* parent)
{
    const char* what = "jump";
    if (!parent) return afail(what, "null pointer");
    if (!faces_ok(F)) return afail(what, "F must be in 1..2^29-1");
    hipLaunchKernelGGL(jump_kernel, grid_of(F), dim3(kThreads), 0, (hipStream_t)stream, F, parent);
    return mesh_launched("atlas", what);
}

int gd_atlas_roots(void* stream, int F, const int32_t* cls, const int32_t* parent, int32_t* is_root)
{
    const char* what = "roots";
    if (!cls || !parent || !is_root) return afail(what, "null pointer");
    if (!faces_ok(F)) return afail(what, "F must be in 1..2^29-1");
    hipLaunchKernelGGL(roots_kernel, grid_of(F), dim3(kThreads), 0, (hipStream_t)stream, F, cls, parent, is_root);
    return mesh_launched("atlas", what);
}

int gd_atlas_bounds(void* stream, int V, int F, int C, const float* verts, const int32_t* tri, const int32_t* cls,
                    const int32_t* parent, const int32_t* scan, int32_t* face_chart, uint32_t* keys, float* bounds,
                    int32_t* count)
{
    const char* what = "bounds";
    if (!verts || !tri || !cls || !parent || !scan || !face_chart || !keys || !bounds || !count)
        return afail(what, "null pointer");
    if (V < 1 || !faces_ok(F) || C < 1 || C > F) return afail(what, "V must be at least 1, F in 1..2^29-1 and C in 1..F");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bounds_init_kernel, grid_of(C), dim3(kThreads), 0, s, C, keys, count);
    hipLaunchKernelGGL(bounds_kernel, grid_of(F), dim3(kThreads), 0, s, V, F, C, verts, tri, cls, parent, scan, face_chart, keys,
                       count);
    hipLaunchKernelGGL(bounds_decode_kernel, grid_of(4 * C), dim3(kThreads), 0, s, 4 * C, keys, bounds);
    return mesh_launched("atlas", what);
}

int gd_atlas_emit(void* stream, int V, int F, int C, int resolution, int gutter, float scale, const float* verts,
                  const int32_t* tri, const int32_t* cls, const int32_t* face_chart, const float* bounds,
                  const int32_t* offsets, int32_t* corner_xy, int64_t* key)
{
    const char* what = "emit";
    if (!verts || !tri || !cls || !face_chart || !bounds || !offsets || !corner_xy || !key) return afail(what, "null pointer");
    if (V < 1 || !faces_ok(F) || C < 1 || C > F) return afail(what, "V must be at least 1, F in 1..2^29-1 and C in 1..F");
    if (resolution < 1 || resolution > GD_ATLAS_MAX_RESOLUTION) return afail(what, "resolution must be in 1..16384");
    if (gutter < 0 || gutter > GD_ATLAS_MAX_GUTTER) return afail(what, "gutter must be in 0..64");
    if (!(scale > 0.0f) || !isfinite(scale)) return afail(what, "scale must be positive and finite");
    hipLaunchKernelGGL(emit_kernel, grid_of(3 * F), dim3(kThreads), 0, (hipStream_t)stream, V, F, C, gutter, scale,
                       verts, tri, cls, face_chart, bounds, offsets, corner_xy, key);
    return mesh_launched("atlas", what);
}

int gd_atlas_write_vt(void* stream, int n, int T, int resolution, const int64_t* row, const int32_t* corner_xy, float* vt,
                      int32_t* ft)
{
    const char* what = "write vt";
    if (!row || !corner_xy || !vt || !ft) return afail(what, "null pointer");
    if (n < 3 || n % 3 != 0 || n / 3 >= kMaxFaces || T < 1 || T > n) return afail(what, "n must be 3F with F in 1..2^29-1 and T in 1..n");
    if (resolution < 1 || resolution > GD_ATLAS_MAX_RESOLUTION) return afail(what, "resolution must be in 1..16384");
    hipLaunchKernelGGL(write_vt_kernel, grid_of(n), dim3(kThreads), 0, (hipStream_t)stream, n, T, (float)(256 * resolution), row,
                       corner_xy, vt, ft);
    return mesh_launched("atlas", what);
}

int gd_atlas_lost_faces(void* stream, int F, int H, int W, const int32_t* corner_xy, const float* rast, int freeze,
                        int32_t* lost, int32_t* layer, int32_t* single)
{
    const char* what = "lost faces";
    if (!corner_xy || !rast || !lost || !layer || !single) return afail(what, "null pointer");
    if (!faces_ok(F)) return afail(what, "F must be in 1..2^29-1");
    if (H < 1 || W < 1 || H > GD_ATLAS_MAX_RESOLUTION || W > GD_ATLAS_MAX_RESOLUTION) return afail(what, "H and W must be in 1..16384");
    hipLaunchKernelGGL(lost_faces_kernel, dim3((unsigned)((F + kLostWaves - 1) / kLostWaves)), dim3(kThreads), 0,
                       (hipStream_t)stream, F, H, W, corner_xy, rast, freeze, lost, layer, single);
    return mesh_launched("atlas", what);
}

}  // extern "C"
