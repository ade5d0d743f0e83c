// raster_mesh.hip -- triangle-mesh render path of the NeTF stage (C-ABI and the DEFINITIONS: include/gd_mesh.h):
// rasterize / interpolate / antialias, the three nvdiffrast operations Renderer.render rests on
// (Garment_Deformer_NeTF/netf/render/mesh_renderer.py:338-428).  Built with -ffp-contract=off: rast and wts are compared
// bit for bit with an fp32 numpy statement (tests/mesh_reference.py).
//
// rasterize is a visibility buffer.  Garment meshes at 512^2 are micro-triangles of a few pixels each, so there is no
// (triangle, tile) binning:
//   raster_small   one thread per triangle: setup, clipped pixel bounding box; a box of <= 256 pixels is walked here,
//                  one 64-bit atomicMin of (order-preserving bits of zw) << 32 | id per covered pixel into a [H][W]
//                  u64 buffer (all ones = empty); a min does not depend on arrival order, so reruns are bit-identical.
//                  Larger boxes are appended to a list of capacity F (it cannot overflow; its ORDER is not
//                  reproducible and does not matter).
//   raster_large   one wave per listed triangle, lanes striding the box; the list length is read on the device.
//   raster_resolve one thread per pixel decodes the winner and recomputes E, b, zw, u, v with the SAME device function
//                  (same bits) and writes one 16-byte store.
// interpolate backward is the store-then-sum form: corner_grad (one wave per triangle, fixed lane-strided order, fixed
// shuffle tree) writes a [F][3][C] slab, vertex_sum adds each vertex's corners in CSR order.  No atomics.
// antialias is a gather: aa_weights analyses each pixel's four pairs once per (rast, pos); aa_apply blends any image
// with those weights, or applies the adjoint.
// Gradients to vertex positions (include/gd_mesh_deform.h, for the mesh deformer): raster_backward and aa_backward_pos
// have the shape of corner_grad, a [F][3][4] slab of (x, y, 0, w) per corner that vertex_sum adds per vertex;
// aa_backward_pos takes each pair's decisions from pair_analyse, the device function aa_weights uses.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_mesh.h"
#include "../../include/gd_mesh_deform.h"
#include "raster_common.h"

namespace gd {
namespace {

thread_local char g_mesh_err[256] = "";

int mfail(int code, const char* msg)
{
    snprintf(g_mesh_err, sizeof(g_mesh_err), "%s", msg);
    return code;
}

constexpr int kSnapLimit = 1 << 24;
constexpr int kLargeWaves = 1024;   // waves of raster_large (256 workgroups of 4)

struct Vert {
    int X, Y;
    float zn, rw;
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e+38f; }

// false: the vertex is unusable (w <= 0, non-finite, or off the 2^24 snap range)
__device__ __forceinline__ bool snap_vertex(const float* __restrict__ pos, int v, int H, int W, Vert& o)
{
    const float4 p = reinterpret_cast<const float4*>(pos)[v];
    if (!(p.w > 0.0f)) return false;
    const float rw = 1.0f / p.w;
    const float xn = p.x * rw, yn = p.y * rw, zn = p.z * rw;
    if (!finite_f(rw) || !finite_f(xn) || !finite_f(yn) || !finite_f(zn)) return false;
    const float fx = rintf((xn * 0.5f + 0.5f) * (float)(256 * W));
    const float fy = rintf((yn * 0.5f + 0.5f) * (float)(256 * H));
    if (!(fabsf(fx) <= (float)kSnapLimit) || !(fabsf(fy) <= (float)kSnapLimit)) return false;
    o.X = (int)fx;
    o.Y = (int)fy;
    o.zn = zn;
    o.rw = rw;
    return true;
}

struct TriSetup {
    Vert v[3];
    int64_t dX[3], dY[3];   // orientation-normalised edge vectors: edge i runs from vertex i+1 to vertex i+2
    int64_t A;              // > 0
    int c0, c1, r0, r1;     // clipped pixel bounding box, inclusive (empty if c0 > c1 or r0 > r1)
};

__device__ __forceinline__ bool setup_triangle(const float* __restrict__ pos, const int* __restrict__ tri, int t, int V,
                                               int H, int W, TriSetup& s)
{
    const int i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
    if (!snap_vertex(pos, i0, H, W, s.v[0]) || !snap_vertex(pos, i1, H, W, s.v[1]) || !snap_vertex(pos, i2, H, W, s.v[2]))
        return false;
    int64_t A = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        s.dX[i] = (int64_t)s.v[k].X - s.v[j].X;
        s.dY[i] = (int64_t)s.v[k].Y - s.v[j].Y;
    }
    // A = E0 + E1 + E2 is the same at every point; at vertex 0, E1 and E2 vanish
    A =s.dX[0] * ((int64_t)s.v[0].Y - s.v[1].Y) - s.dY[0] * ((int64_t)s.v[0].X - s.v[1].X);
    if (A == 0) return false;
    if (A < 0) {
        A = -A;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            s.dX[i] = -s.dX[i];
            s.dY[i] = -s.dY[i];
        }
    }
    s.A = A;
    const int xmin = min(s.v[0].X, min(s.v[1].X, s.v[2].X)), xmax = max(s.v[0].X, max(s.v[1].X, s.v[2].X));
    const int ymin = min(s.v[0].Y, min(s.v[1].Y, s.v[2].Y)), ymax = max(s.v[0].Y, max(s.v[1].Y, s.v[2].Y));
    // centres 256 c + 128 inside [xmin, xmax]; >> 8 of a negative int is the floor
    s.c0 = max((xmin - 128 + 255) >> 8, 0);
    s.c1 = min((xmax - 128) >> 8, W - 1);
    s.r0 = max((ymin - 128 + 255) >> 8, 0);
    s.r1 = min((ymax - 128) >> 8, H - 1);
    return true;
}

// edge functions at the centre of pixel (r, c); true if covered
__device__ __forceinline__ bool edges_at(const TriSetup& s, int r, int c, int64_t E[3])
{
    const int64_t Px = 256 * (int64_t)c + 128, Py = 256 * (int64_t)r + 128;
    bool in = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3;
        E[i] = s.dX[i] * (Py - s.v[j].Y) - s.dY[i] * (Px - s.v[j].X);
        in = in && (E[i] > 0 || (E[i] == 0 && (s.dY[i] > 0 || (s.dY[i] == 0 && s.dX[i] < 0))));
    }
    return in;
}

// (u, v, zw) of a covered pixel; false if zw is outside [-1, 1]
__device__ __forceinline__ bool shade(const TriSetup& s, const int64_t E[3], float& u, float& v, float& zw)
{
    const float fa = (float)s.A;
    const float b0 = (float)E[0] / fa, b1 = (float)E[1] / fa, b2 = (float)E[2] / fa;
    float z = (b0 * s.v[0].zn + b1 * s.v[1].zn) + b2 * s.v[2].zn;
    if (z == 0.0f) z = 0.0f;   // -0 -> +0
    if (!(z >= -1.0f && z <= 1.0f)) return false;
    const float p0 = b0 * s.v[0].rw, p1 = b1 * s.v[1].rw, p2 = b2 * s.v[2].rw;
    const float sum = (p0 + p1) + p2;
    u = p0 / sum;
    v = p1 / sum;
    zw = z;
    return true;
}

__device__ __forceinline__ uint32_t depth_bits(float zw)
{
    const uint32_t b = __float_as_uint(zw);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ void raster_pixel(const TriSetup& s, int t, int r, int c, int W,
                                             unsigned long long* __restrict__ vis)
{
    int64_t E[3];
    if (!edges_at(s, r, c, E)) return;
    float u, v, zw;
    if (!shade(s, E, u, v, zw)) return;
    atomicMin(&vis[(size_t)r * W + c], ((unsigned long long)depth_bits(zw) << 32) | (uint32_t)t);
}

__global__ __launch_bounds__(256) void raster_small_kernel(int V, int F, int H, int W, const float* __restrict__ pos,
                                                           const int* __restrict__ tri,
                                                           unsigned long long* __restrict__ vis,
                                                           uint32_t* __restrict__ large_count, int* __restrict__ large_list)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= F) return;
    TriSetup s;
    if (!setup_triangle(pos, tri, t, V, H, W, s)) return;
    if (s.c0 > s.c1 || s.r0 > s.r1) return;
    const int bw = s.c1 - s.c0 + 1, bh = s.r1 - s.r0 + 1;
    if ((int64_t)bw * bh > GD_MESH_LARGE_BOX) {
        const uint32_t slot = atomicAdd(large_count, 1u);
        if (slot < (uint32_t)F) large_list[slot] = t;
        return;
    }
    for (int r = s.r0; r <= s.r1; r++)
        for (int c = s.c0; c <= s.c1; c++) raster_pixel(s, t, r, c, W, vis);
}

__global__ __launch_bounds__(256) void raster_large_kernel(int V, int F, int H, int W, const float* __restrict__ pos,
                                                           const int* __restrict__ tri,
                                                           unsigned long long* __restrict__ vis,
                                                           const uint32_t* __restrict__ large_count,
                                                           const int* __restrict__ large_list)
{
    const int lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t n = min(*large_count, (uint32_t)F);
    for (uint32_t i = wave; i < n; i += kLargeWaves) {
        const int t = large_list[i];
        TriSetup s;
        if ((unsigned)t >= (unsigned)F || !setup_triangle(pos, tri, t, V, H, W, s)) continue;
        const int bw = s.c1 - s.c0 + 1, bh = s.r1 - s.r0 + 1;
        if (bw <= 0 || bh <= 0) continue;
        const int64_t npix = (int64_t)bw * bh;
        for (int64_t q = lane; q < npix; q += 64) raster_pixel(s, t, s.r0 + (int)(q / bw), s.c0 + (int)(q % bw), W, vis);
    }
}

__global__ __launch_bounds__(256) void raster_resolve_kernel(int V, int F, int H, int W, const float* __restrict__ pos,
                                                             const int* __restrict__ tri,
                                                             const unsigned long long* __restrict__ vis,
                                                             float4* __restrict__ rast)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const unsigned long long key = vis[p];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int t = (int)(uint32_t)(key & 0xffffffffull);
    if (key != ~0ull && (unsigned)t < (unsigned)F) {
        TriSetup s;
        int64_t E[3];
        float u, v, zw;
        if (setup_triangle(pos, tri, t, V, H, W, s) && edges_at(s, p / W, p % W, E) && shade(s, E, u, v, zw))
            o = make_float4(u, v, zw, (float)(t + 1));
    }
    rast[p] = o;
}

// ---- interpolate -----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void interp_forward_kernel(int V, int F, int C, int npix, const float* __restrict__ attr,
                                                             const float4* __restrict__ rast, const int* __restrict__ tri,
                                                             float* __restrict__ out)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const float4 ra = rast[p];
    const int t = (int)ra.w - 1;
    float* o = out + (size_t)p * C;
    int i0 = 0, i1 = 0, i2 = 0;
    bool ok = t >= 0 && t < F;
    if (ok) {
        i0 = tri[3 * (size_t)t];
        i1 = tri[3 * (size_t)t + 1];
        i2 = tri[3 * (size_t)t + 2];
        ok = (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
    }
    if (!ok) {
        for (int k = 0; k < C; k++) o[k] = 0.0f;
        return;
    }
    const float u = ra.x, v = ra.y, w = (1.0f - u) - v;
    for (int k = 0; k < C; k++)
        o[k] = (u * attr[(size_t)i0 * C + k] + v * attr[(size_t)i1 * C + k]) + w * attr[(size_t)i2 * C + k];
}

// one wave per triangle; slab[t][i][k] = sum over the triangle's visible pixels of weight_i * dout[k]
__global__ __launch_bounds__(256) void corner_grad_kernel(int V, int F, int C, int H, int W, const float* __restrict__ pos,
                                                          const int* __restrict__ tri, const float4* __restrict__ rast,
                                                          const float* __restrict__ dout, float* __restrict__ slab)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= F) return;
    float g[3][GD_MESH_MAX_CHANNELS];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < GD_MESH_MAX_CHANNELS; k++) g[i][k] = 0.0f;
    TriSetup s;
    if (setup_triangle(pos, tri, t, V, H, W, s) && s.c0 <= s.c1 && s.r0 <= s.r1) {
        const int bw = s.c1 - s.c0 + 1, bh = s.r1 - s.r0 + 1;
        const int64_t npix = (int64_t)bw * bh;
        const float id = (float)(t + 1);
        for (int64_t q = lane; q < npix; q += 64) {
            const size_t p = (size_t)(s.r0 + (int)(q / bw)) * W + (s.c0 + (int)(q % bw));
            const float4 ra = rast[p];
            if (ra.w != id) continue;
            const float w2 = (1.0f - ra.x) - ra.y;
#pragma unroll
            for (int k = 0; k < GD_MESH_MAX_CHANNELS; k++) {
                if (k < C) {
                    const float d = dout[p * C + k];
                    g[0][k] += ra.x * d;
                    g[1][k] += ra.y * d;
                    g[2][k] += w2 * d;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < GD_MESH_MAX_CHANNELS; k++) {
            if (k < C) {
                float x = g[i][k];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
                if (lane == 0) slab[((size_t)t * 3 + i) * C + k] = x;
            }
        }
}

__global__ __launch_bounds__(256) void vertex_sum_kernel(int V, int F, int C, const int* __restrict__ corner_ptr,
                                                         const int* __restrict__ corner_idx,
                                                         const float* __restrict__ slab, float* __restrict__ dattr)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)V * C) return;
    const int v = (int)(e / C), k = (int)(e % C);
    const int a = max(corner_ptr[v], 0), b = min(corner_ptr[v + 1], 3 * F);
    float sum = 0.0f;
    for (int j = a; j < b; j++) {
        const int corner = corner_idx[j];
        if ((unsigned)corner < (unsigned)(3 * F)) sum += slab[(size_t)corner * C + k];
    }
    dattr[e] = sum;
}

// ---- antialias -------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int sign64(int64_t x) { return (x > 0) - (x < 0); }

// what the analysis of one pair decided (edge < 0: no silhouette edge with t <= 1, no weight)
struct PairInfo {
    int t;             // the chosen triangle
    int edge;          // its deciding edge, running from corner edge + 1 to corner edge + 2
    bool p_is_inner;   // p is the chosen triangle's pixel I
    float tt;          // crossing distance from I's centre, from the snapped vertices
};

// the pair of pixel p = (r, c) and its neighbour n = (rn, cn); horizontal: the pair lies in one row.  The one place the
// pair's decisions are taken: aa_weights_kernel and aa_backward_pos_kernel both read them here.
__device__ __forceinline__ bool pair_analyse(int V, int F, int H, int W, const float4* __restrict__ rast,
                                             const float* __restrict__ pos, const int* __restrict__ tri,
                                             const int* __restrict__ opp, int r, int c, int rn, int cn, bool horizontal,
                                             const float4& rp, PairInfo& o)
{
    o.edge = -1;
    const float4 rq = rast[(size_t)rn * W + cn];
    const int idp = (int)rp.w, idn = (int)rq.w;
    if (idp == idn) return false;
    bool p_is_inner;
    if (idp == 0) p_is_inner = false;
    else if (idn == 0) p_is_inner = true;
    else if (rp.z != rq.z) p_is_inner = rp.z < rq.z;
    else p_is_inner = idp < idn;
    const int t = (p_is_inner ? idp : idn) - 1;
    if ((unsigned)t >= (unsigned)F) return false;
    o.t = t;
    o.p_is_inner = p_is_inner;
    const int ri = p_is_inner ? r : rn, ci = p_is_inner ? c : cn;
    int vi[3];
    Vert vv[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        vi[i] = tri[3 * (size_t)t + i];
        if ((unsigned)vi[i] >= (unsigned)V || !snap_vertex(pos, vi[i], H, W, vv[i])) return false;
    }
    // the line through the two centres, in sub-pixel units: y = L for a horizontal pair, x = L for a vertical one
    const int L = horizontal ? 256 * r + 128 : 256 * c + 128;
    const float line = (horizontal ? (float)r : (float)c) + 0.5f;
    const float centre = (horizontal ? (float)ci : (float)ri) + 0.5f;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const Vert& a = vv[(i + 1) % 3];
        const Vert& b = vv[(i + 2) % 3];
        const Vert& cc = vv[i];
        const int d = opp[3 * (size_t)t + i];
        bool sil = d < 0 || d >= V;
        if (!sil) {
            Vert dv;
            if (!snap_vertex(pos, d, H, W, dv)) sil = true;
            else {
                const int64_t ex = (int64_t)b.X - a.X, ey = (int64_t)b.Y - a.Y;
                const int sc = sign64(ex * ((int64_t)cc.Y - a.Y) - ey * ((int64_t)cc.X - a.X));
                const int sd = sign64(ex * ((int64_t)dv.Y - a.Y) - ey * ((int64_t)dv.X - a.X));
                sil = sc * sd >= 0;
            }
        }
        if (!sil) continue;
        const int a_on = horizontal ? a.Y : a.X, b_on = horizontal ? b.Y : b.X;       // coordinate across the line
        if ((a_on <= L) == (b_on <= L)) continue;
        const float sa_on = (float)a_on / 256.0f, sb_on = (float)b_on / 256.0f;
        const float sa_al = (float)(horizontal ? a.X : a.Y) / 256.0f, sb_al = (float)(horizontal ? b.X : b.Y) / 256.0f;
        const float x = sa_al + (sb_al - sa_al) * ((line - sa_on) / (sb_on - sa_on));
        const float tt = fabsf(x - centre);
        if (!(tt <= 1.0f)) continue;
        o.edge = i;
        o.tt = tt;
        return true;
    }
    return false;
}

// weight pixel p = (r, c) receives from its neighbour n = (rn, cn)
__device__ __forceinline__ float pair_weight(int V, int F, int H, int W, const float4* __restrict__ rast,
                                             const float* __restrict__ pos, const int* __restrict__ tri,
                                             const int* __restrict__ opp, int r, int c, int rn, int cn, bool horizontal,
                                             const float4& rp)
{
    PairInfo o;
    if (!pair_analyse(V, F, H, W, rast, pos, tri, opp, r, c, rn, cn, horizontal, rp, o)) return 0.0f;
    if (o.tt > 0.5f) return o.p_is_inner ? 0.0f : o.tt - 0.5f;
    return o.p_is_inner ? 0.5f - o.tt : 0.0f;
}

__global__ __launch_bounds__(256) void aa_weights_kernel(int V, int F, int H, int W, const float4* __restrict__ rast,
                                                         const float* __restrict__ pos, const int* __restrict__ tri,
                                                         const int* __restrict__ opp, float4* __restrict__ wts)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= H * W) return;
    const int r = p / W, c = p % W;
    const float4 rp = rast[p];
    float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (c > 0) w.x = pair_weight(V, F, H, W, rast, pos, tri, opp, r, c, r, c - 1, true, rp);
    if (c < W - 1) w.y = pair_weight(V, F, H, W, rast, pos, tri, opp, r, c, r, c + 1, true, rp);
    if (r > 0) w.z = pair_weight(V, F, H, W, rast, pos, tri, opp, r, c, r - 1, c, false, rp);
    if (r < H - 1) w.w = pair_weight(V, F, H, W, rast, pos, tri, opp, r, c, r + 1, c, false, rp);
    wts[p] = w;
}

__global__ __launch_bounds__(256) void aa_apply_kernel(int C, int H, int W, const float* __restrict__ in,
                                                       const float4* __restrict__ wts, float* __restrict__ out,
                                                       int adjoint)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)H * W * C) return;
    const int p = (int)(e / C), k = (int)(e % C);
    const int r = p / W, c = p % W;
    const float4 w4 = wts[p];
    const float w[4] = {w4.x, w4.y, w4.z, w4.w};
    const int nb[4] = {c > 0 ? p - 1 : -1, c < W - 1 ? p + 1 : -1, r > 0 ? p - W : -1, r < H - 1 ? p + W : -1};
    const float x = in[e];
    float acc;
    if (!adjoint) {
        acc = x;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (nb[j] >= 0 && w[j] != 0.0f) acc += w[j] * (in[(size_t)nb[j] * C + k] - x);
    } else {
        acc = x * (1.0f - (((w[0] + w[1]) + w[2]) + w[3]));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (nb[j] < 0) continue;
            const float4 wn = wts[nb[j]];
            const float back = j == 0 ? wn.y : j == 1 ? wn.x : j == 2 ? wn.w : wn.z;   // the neighbour's weight from p
            if (back != 0.0f) acc += back * in[(size_t)nb[j] * C + k];
        }
    }
    out[e] = acc;
}

// ---- gradients to vertex positions (include/gd_mesh_deform.h; definitions: include/gd_mesh.h) --------------------------
// The forward's discrete decisions are held fixed and the snapping is removed: the derivatives are those of the
// continuous functions of the fp32 clip positions.  Both position gradients keep the shape of corner_grad + vertex_sum:
// one wave per triangle walks the triangle's pixel box, keeps the pixels whose rast id is this triangle, reduces nine
// values (x, y, w of three corners) with the fixed shuffle tree into a [F][3][4] slab; vertex_sum adds it per vertex.

// drast[p] = (sum_k dout_k (a0_k - a2_k), sum_k dout_k (a1_k - a2_k), 0, 0); zeros on background
__global__ __launch_bounds__(256) void interp_backward_rast_kernel(int V, int F, int C, int npix,
                                                                   const float* __restrict__ attr,
                                                                   const float4* __restrict__ rast,
                                                                   const int* __restrict__ tri,
                                                                   const float* __restrict__ dout,
                                                                   float4* __restrict__ drast)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int t = (int)rast[p].w - 1;
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (t >= 0 && t < F) {
        const int i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
        if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
            for (int k = 0; k < C; k++) {
                const float d = dout[(size_t)p * C + k], a2 = attr[(size_t)i2 * C + k];
                o.x += d * (attr[(size_t)i0 * C + k] - a2);
                o.y += d * (attr[(size_t)i1 * C + k] - a2);
            }
        }
    }
    drast[p] = o;
}

// lane-local sums of one wave -> slab[t][i] = (x, y, 0, w), the same tree as corner_grad_kernel
__device__ __forceinline__ void store_corner_slab(float g[3][3], int t, int lane, float4* __restrict__ slab)
{
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float x = g[i][j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
            g[i][j] = x;
        }
        if (lane == 0) slab[(size_t)t * 3 + i] = make_float4(g[i][0], g[i][1], 0.0f, g[i][2]);
    }
}

__global__ __launch_bounds__(256) void raster_backward_kernel(int V, int F, int H, int W, const float* __restrict__ pos,
                                                              const int* __restrict__ tri,
                                                              const float4* __restrict__ rast,
                                                              const float4* __restrict__ drast, float4* __restrict__ slab)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= F) return;
    float g[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) g[i][j] = 0.0f;
    TriSetup s;
    if (setup_triangle(pos, tri, t, V, H, W, s) && s.c0 <= s.c1 && s.r0 <= s.r1) {
        float4 P[3];   // the indices are in range: setup_triangle checked them
#pragma unroll
        for (int i = 0; i < 3; i++) P[i] = reinterpret_cast<const float4*>(pos)[tri[3 * (size_t)t + i]];
        const int bw = s.c1 - s.c0 + 1, bh = s.r1 - s.r0 + 1;
        const int64_t npix = (int64_t)bw * bh;
        const float id = (float)(t + 1);
        for (int64_t q = lane; q < npix; q += 64) {
            const int r = s.r0 + (int)(q / bw), c = s.c0 + (int)(q % bw);
            const size_t p = (size_t)r * W + c;
            if (rast[p].w != id) continue;
            const float4 d = drast[p];
            const float fx = (float)(2 * c + 1) / (float)W - 1.0f, fy = (float)(2 * r + 1) / (float)H - 1.0f;
            float qx[3], qy[3];
#pragma unroll
            for (int i = 0; i < 3; i++) {
                qx[i] = P[i].x - fx * P[i].w;
                qy[i] = P[i].y - fy * P[i].w;
            }
            const float a0 = qx[1] * qy[2] - qy[1] * qx[2];
            const float a1 = qx[2] * qy[0] - qy[2] * qx[0];
            const float a2 = qx[0] * qy[1] - qy[0] * qx[1];
            const float S = (a0 + a1) + a2;
            if (S == 0.0f || !finite_f(S)) continue;
            const float u = a0 / S, v = a1 / S;
            const float m = d.x * u + d.y * v;
            const float g0 = (d.x - m) / S, g1 = (d.y - m) / S, g2 = -m / S;   // dL/da_i
            const float dqx[3] = {g2 * qy[1] - g1 * qy[2], g0 * qy[2] - g2 * qy[0], g1 * qy[0] - g0 * qy[1]};
            const float dqy[3] = {g1 * qx[2] - g2 * qx[1], g2 * qx[0] - g0 * qx[2], g0 * qx[1] - g1 * qx[0]};
#pragma unroll
            for (int i = 0; i < 3; i++) {
                g[i][0] += dqx[i];
                g[i][1] += dqy[i];
                g[i][2] += -(fx * dqx[i]) - fy * dqy[i];
            }
        }
    }
    store_corner_slab(g, t, lane, slab);
}

__global__ __launch_bounds__(256) void aa_backward_pos_kernel(int V, int F, int C, int H, int W,
                                                              const float4* __restrict__ rast,
                                                              const float* __restrict__ pos, const int* __restrict__ tri,
                                                              const int* __restrict__ opp, const float* __restrict__ in,
                                                              const float* __restrict__ dout, float4* __restrict__ slab)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= F) return;
    float g[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) g[i][j] = 0.0f;
    TriSetup s;
    if (setup_triangle(pos, tri, t, V, H, W, s) && s.c0 <= s.c1 && s.r0 <= s.r1) {
        float4 P[3];
#pragma unroll
        for (int i = 0; i < 3; i++) P[i] = reinterpret_cast<const float4*>(pos)[tri[3 * (size_t)t + i]];
        const int bw = s.c1 - s.c0 + 1, bh = s.r1 - s.r0 + 1;
        const int64_t npix = (int64_t)bw * bh;
        const float id = (float)(t + 1);
        const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
        for (int64_t q = lane; q < npix; q += 64) {
            const int r = s.r0 + (int)(q / bw), c = s.c0 + (int)(q % bw);
            const size_t p = (size_t)r * W + c;
            const float4 rp = rast[p];
            if (rp.w != id) continue;
            // the pixel's four pairs in the order of wts; a pair counts here only if this pixel is its I
            for (int k = 0; k < 4; k++) {
                const bool horizontal = k < 2;
                const int rn = r + (k == 2 ? -1 : k == 3 ? 1 : 0), cn = c + (k == 0 ? -1 : k == 1 ? 1 : 0);
                if (rn < 0 || rn >= H || cn < 0 || cn >= W) continue;
                PairInfo o;
                if (!pair_analyse(V, F, H, W, rast, pos, tri, opp, r, c, rn, cn, horizontal, rp, o) || !o.p_is_inner)
                    continue;
                const size_t n = (size_t)rn * W + cn;
                const bool onto_outer = o.tt > 0.5f;
                float dw = 0.0f;
                if (onto_outer)
                    for (int ch = 0; ch < C; ch++) dw += dout[n * C + ch] * (in[p * C + ch] - in[n * C + ch]);
                else
                    for (int ch = 0; ch < C; ch++) dw += dout[p * C + ch] * (in[n * C + ch] - in[p * C + ch]);
                const float dt = onto_outer ? dw : -dw;
                const int e = o.edge;
                const float4 pa = e == 0 ? P[1] : e == 1 ? P[2] : P[0];
                const float4 pb = e == 0 ? P[2] : e == 1 ? P[0] : P[1];
                const float sxa = (pa.x / pa.w * 0.5f + 0.5f) * (float)W, sya = (pa.y / pa.w * 0.5f + 0.5f) * (float)H;
                const float sxb = (pb.x / pb.w * 0.5f + 0.5f) * (float)W, syb = (pb.y / pb.w * 0.5f + 0.5f) * (float)H;
                const float al_a = horizontal ? sxa : sya, on_a = horizontal ? sya : sxa;
                const float al_b = horizontal ? sxb : syb, on_b = horizontal ? syb : sxb;
                const float line = (horizontal ? (float)r : (float)c) + 0.5f;
                const float centre = (horizontal ? (float)c : (float)r) + 0.5f;
                const float D = on_b - on_a;
                if (D == 0.0f || !finite_f(D)) continue;
                const float sp = (line - on_a) / D;
                const float x = al_a + (al_b - al_a) * sp;
                const float gx = x > centre ? dt : x < centre ? -dt : 0.0f;     // dL/dx*
                const float d_al_a = gx * (1.0f - sp), d_al_b = gx * sp;
                const float ds = gx * (al_b - al_a);
                const float d_on_a = ds * (sp - 1.0f) / D, d_on_b = -(ds * sp) / D;
                const float dsxa = horizontal ? d_al_a : d_on_a, dsya = horizontal ? d_on_a : d_al_a;
                const float dsxb = horizontal ? d_al_b : d_on_b, dsyb = horizontal ? d_on_b : d_al_b;
                const float ga[3] = {dsxa * hw / pa.w, dsya * hh / pa.w,
                                     -(dsxa * hw * pa.x + dsya * hh * pa.y) / (pa.w * pa.w)};
                const float gb[3] = {dsxb * hw / pb.w, dsyb * hh / pb.w,
                                     -(dsxb * hw * pb.x + dsyb * hh * pb.y) / (pb.w * pb.w)};
                const int ca = e == 2 ? 0 : e + 1, cb = e == 0 ? 2 : e - 1;      // corners (e + 1) % 3 and (e + 2) % 3
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        if (i == ca) g[i][j] += ga[j];
                        if (i == cb) g[i][j] += gb[j];
                    }
            }
        }
    }
    store_corner_slab(g, t, lane, slab);
}

__global__ __launch_bounds__(256) void visible_vertices_kernel(int V, int F, int npix, const float4* __restrict__ rast,
                                                               const int* __restrict__ tri, uint8_t* __restrict__ vis)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    const int t = (int)rast[p].w - 1;
    if (t < 0 || t >= F) return;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int v = tri[3 * (size_t)t + i];
        if ((unsigned)v < (unsigned)V) vis[v] = 1;
    }
}

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

struct RasterScratch {
    uint32_t* large_count;
    unsigned long long* vis;
    int* large_list;
    size_t vis_bytes, total;
};

RasterScratch carve_raster(char* base, int F, int H, int W)
{
    RasterScratch c;
    size_t off = 0;
    c.large_count = (uint32_t*)(base + off); off = align_up(off + sizeof(uint32_t));
    c.vis_bytes = (size_t)(H > 0 ? H : 0) * (size_t)(W > 0 ? W : 0) * sizeof(unsigned long long);
    c.vis = (unsigned long long*)(base + off); off = align_up(off + c.vis_bytes);
    c.large_list = (int*)(base + off); off = align_up(off + (size_t)(F > 0 ? F : 0) * sizeof(int));
    c.total = off;
    return c;
}

const char* check_frame(int H, int W)
{
    if (H <= 0 || W <= 0) return "mesh: H and W must be positive";
    if (H > 8192 || W > 8192) return "mesh: H and W must be <= 8192";
    return nullptr;
}

}  // namespace

int mesh_fail(int code, const char* msg) { return mfail(code, msg); }

int mesh_launched(const char* family, const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    const bool plain = !family || !*family;
    char buf[200];
    snprintf(buf, sizeof(buf), "%s%s%s: %s", plain ? "" : family, plain ? "" : " ", what, hipGetErrorString(e));
    return mfail(-2, buf);
}

}  // namespace gd

extern "C" {

size_t gd_mesh_rasterize_scratch_bytes(int F, int H, int W) { return gd::carve_raster(nullptr, F, H, W).total; }

int gd_mesh_rasterize(void* stream, int V, int F, int H, int W, const float* pos, const int* tri, float* rast,
                      void* scratch)
{
    using namespace gd;
    if (const char* err = check_frame(H, W)) return mfail(-1, err);
    if (V < 0 || F < 0) return mfail(-1, "rasterize: V and F must be >= 0");
    if (F >= (1 << 24)) return mfail(-1, "rasterize: F must be < 2^24 (the id is stored as a float)");
    if (!rast || !scratch || (F > 0 && (!pos || !tri))) return mfail(-1, "rasterize: null pointer");
    hipStream_t s = (hipStream_t)stream;
    RasterScratch c = carve_raster((char*)scratch, F, H, W);
    hipError_t e = hipMemsetAsync(c.large_count, 0, sizeof(uint32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(c.vis, 0xff, c.vis_bytes, s);
    if (e != hipSuccess) return mfail(-2, hipGetErrorString(e));
    if (F > 0) {
        hipLaunchKernelGGL(raster_small_kernel, dim3((F + 255) / 256), dim3(256), 0, s, V, F, H, W, pos, tri, c.vis,
                           c.large_count, c.large_list);
        hipLaunchKernelGGL(raster_large_kernel, dim3(kLargeWaves / 4), dim3(256), 0, s, V, F, H, W, pos, tri, c.vis,
                           c.large_count, c.large_list);
    }
    hipLaunchKernelGGL(raster_resolve_kernel, dim3((H * W + 255) / 256), dim3(256), 0, s, V, F, H, W, pos, tri, c.vis,
                       (float4*)rast);
    return mesh_launched(nullptr, "rasterize");
}

int gd_mesh_interpolate_forward(void* stream, int V, int F, int C, int H, int W, const float* attr, const float* rast,
                                const int* tri, float* out)
{
    using namespace gd;
    if (const char* err = check_frame(H, W)) return mfail(-1, err);
    if (V < 0 || F < 0) return mfail(-1, "interpolate: V and F must be >= 0");
    if (C < 1 || C > GD_MESH_MAX_CHANNELS) return mfail(-1, "interpolate: C must be in [1, 8]");
    if (!rast || !out || (F > 0 && (!attr || !tri))) return mfail(-1, "interpolate: null pointer");
    hipLaunchKernelGGL(interp_forward_kernel, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, V, F, C, H * W,
                       attr, (const float4*)rast, tri, out);
    return mesh_launched(nullptr, "interpolate forward");
}

size_t gd_mesh_interpolate_backward_scratch_bytes(int F, int C)
{
    if (F < 0 || C < 0) return 0;
    return gd::align_up((size_t)F * 3 * (size_t)C * sizeof(float));
}

int gd_mesh_interpolate_backward(void* stream, int V, int F, int C, int H, int W, const float* pos, const int* tri,
                                 const float* rast, const float* dout, const int* corner_ptr, const int* corner_idx,
                                 float* dattr, void* scratch)
{
    using namespace gd;
    if (const char* err = check_frame(H, W)) return mfail(-1, err);
    if (V < 0 || F < 0) return mfail(-1, "interpolate: V and F must be >= 0");
    if (C < 1 || C > GD_MESH_MAX_CHANNELS) return mfail(-1, "interpolate: C must be in [1, 8]");
    if (V == 0) return 0;
    if (!rast || !dout || !dattr || !corner_ptr || (F > 0 && (!pos || !tri || !corner_idx || !scratch)))
        return mfail(-1, "interpolate: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (F > 0)
        hipLaunchKernelGGL(corner_grad_kernel, dim3((F + 3) / 4), dim3(256), 0, s, V, F, C, H, W, pos, tri,
                           (const float4*)rast, dout, (float*)scratch);
    const int64_t n = (int64_t)V * C;
    hipLaunchKernelGGL(vertex_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, V, F, C, corner_ptr,
                       corner_idx, (const float*)scratch, dattr);
    return mesh_launched(nullptr, "interpolate backward");
}

int gd_mesh_antialias_weights(void* stream, int V, int F, int H, int W, const float* rast, const float* pos,
                              const int* tri, const int* opp, float* wts)
{
    using namespace gd;
    if (const char* err = check_frame(H, W)) return mfail(-1, err);
    if (V < 0 || F < 0) return mfail(-1, "antialias: V and F must be >= 0");
    if (!rast || !wts || (F > 0 && (!pos || !tri || !opp))) return mfail(-1, "antialias: null pointer");
    hipLaunchKernelGGL(aa_weights_kernel, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, V, F, H, W,
                       (const float4*)rast, pos, tri, opp, (float4*)wts);
    return mesh_launched(nullptr, "antialias weights");
}

int gd_mesh_antialias_apply(void* stream, int C, int H, int W, const float* in, const float* wts, float* out, int adjoint)
{
    using namespace gd;
    if (const char* err = check_frame(H, W)) return mfail(-1, err);
    if (C < 1 || C > 4096) return mfail(-1, "antialias: C must be in [1, 4096]");
    if (!in || !wts || !out) return mfail(-1, "antialias: null pointer");
    if (in == out) return mfail(-1, "antialias: in and out must not alias");
    const int64_t n = (int64_t)H * W * C;
    hipLaunchKernelGGL(aa_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, C, H, W, in,
                       (const float4*)wts, out, adjoint);
    return mesh_launched(nullptr, "antialias apply");
}

// ---- include/gd_mesh_deform.h ------------------------------------------------------------------------------------------

int gd_mesh_interpolate_backward_rast(void* stream, int V, int F, int C, int H, int W, const float* attr,
                                      const float* rast, const int* tri, const float* dout, float* drast)
{
    using namespace gd;
    if (const char* err = check_frame(H, W)) return mfail(-1, err);
    if (V < 0 || F < 0) return mfail(-1, "interpolate: V and F must be >= 0");
    if (C < 1 || C > GD_MESH_MAX_CHANNELS) return mfail(-1, "interpolate: C must be in [1, 8]");
    if (!rast || !dout || !drast || (F > 0 && (!attr || !tri))) return mfail(-1, "interpolate: null pointer");
    hipLaunchKernelGGL(interp_backward_rast_kernel, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, V, F, C,
                       H * W, attr, (const float4*)rast, tri, dout, (float4*)drast);
    return mesh_launched(nullptr, "interpolate backward (rast)");
}

size_t gd_mesh_rasterize_backward_scratch_bytes(int F)
{
    if (F < 0) return 0;
    return gd::align_up((size_t)F * 3 * 4 * sizeof(float));
}

int gd_mesh_rasterize_backward(void* stream, int V, int F, int H, int W, const float* pos, const int* tri,
                               const float* rast, const float* drast, const int* corner_ptr, const int* corner_idx,
                               float* dpos, void* scratch)
{
    using namespace gd;
    if (const char* err = check_frame(H, W)) return mfail(-1, err);
    if (V < 0 || F < 0) return mfail(-1, "rasterize backward: V and F must be >= 0");
    if (V == 0) return 0;
    if (!rast || !drast || !dpos || !corner_ptr || (F > 0 && (!pos || !tri || !corner_idx || !scratch)))
        return mfail(-1, "rasterize backward: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (F > 0)
        hipLaunchKernelGGL(raster_backward_kernel, dim3((F + 3) / 4), dim3(256), 0, s, V, F, H, W, pos, tri,
                           (const float4*)rast, (const float4*)drast, (float4*)scratch);
    const int64_t n = (int64_t)V * 4;
    hipLaunchKernelGGL(vertex_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, V, F, 4, corner_ptr,
                       corner_idx, (const float*)scratch, dpos);
    return mesh_launched(nullptr, "rasterize backward");
}

size_t gd_mesh_antialias_backward_pos_scratch_bytes(int F) { return gd_mesh_rasterize_backward_scratch_bytes(F); }

int gd_mesh_antialias_backward_pos(void* stream, int V, int F, int C, int H, int W, const float* rast, const float* pos,
                                   const int* tri, const int* opp, const float* in, const float* dout,
                                   const int* corner_ptr, const int* corner_idx, float* dpos, void* scratch)
{
    using namespace gd;
    if (const char* err = check_frame(H, W)) return mfail(-1, err);
    if (V < 0 || F < 0) return mfail(-1, "antialias backward: V and F must be >= 0");
    if (C < 1 || C > 4096) return mfail(-1, "antialias: C must be in [1, 4096]");
    if (V == 0) return 0;
    if (!rast || !in || !dout || !dpos || !corner_ptr || (F > 0 && (!pos || !tri || !opp || !corner_idx || !scratch)))
        return mfail(-1, "antialias backward: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (F > 0)
        hipLaunchKernelGGL(aa_backward_pos_kernel, dim3((F + 3) / 4), dim3(256), 0, s, V, F, C, H, W, (const float4*)rast,
                           pos, tri, opp, in, dout, (float4*)scratch);
    const int64_t n = (int64_t)V * 4;
    hipLaunchKernelGGL(vertex_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, V, F, 4, corner_ptr,
                       corner_idx, (const float*)scratch, dpos);
    return mesh_launched(nullptr, "antialias backward (pos)");
}

int gd_mesh_visible_vertices(void* stream, int V, int F, int npix, const float* rast, const int* tri, uint8_t* vis)
{
    using namespace gd;
    if (V < 0 || F < 0) return mfail(-1, "visible vertices: V and F must be >= 0");
    if (npix <= 0 || npix > 8192 * 8192) return mfail(-1, "visible vertices: npix must be in [1, 8192^2]");
    if (V == 0 || F == 0) return 0;
    if (!rast || !tri || !vis) return mfail(-1, "visible vertices: null pointer");
    hipLaunchKernelGGL(visible_vertices_kernel, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream, V, F, npix,
                       (const float4*)rast, tri, vis);
    return mesh_launched(nullptr, "visible vertices");
}

const char* gd_mesh_last_error(void) { return gd::g_mesh_err; }

}  // extern "C"
