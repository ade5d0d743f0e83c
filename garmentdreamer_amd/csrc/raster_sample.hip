// raster_sample.hip -- texture sampling for the mesh path (C-ABI and the DEFINITIONS: include/gd_sample.h): the
// screen-space derivatives of the rasterizer's (u, v) and of interpolated attributes, the mip pyramid, the four filter
// modes and the gradient to the texture.  fp32 without contraction, every operation in the header's order; no float
// atomics; nothing waits for the device.
//
//   rast_db, interpolate_da   one thread per pixel.
//   build mips                one thread per texel: level 0 is the texture padded to 16-byte texels, then one launch per
//                             level, each reading the level before it.
//   forward                   a gather bound on memory: one thread per pixel, every tap ONE 16-byte load of a padded
//                             texel, all taps of a pixel (4, or 8 for the trilinear mode) issued before the first use so
//                             that a wave keeps 256-512 loads in flight.  Neighbouring pixels of a render read
//                             neighbouring texels, so the taps of a wave fall into a few cache lines and the coarser
//                             levels stay in L2; nothing is staged in LDS because no pixel knows its neighbours' texels
//                             before it has computed its own.
//   items                     one thread per pixel writes its T keys and T x C values with plain stores.
//   reduce                    one thread per sorted position; the first of a run walks the run in order.  A run is as long
//                             as the number of pixels that touch one texel: a handful at render-like level selection,
//                             the whole image for the 1 x 1 top level, which then is one thread's serial sum.
//   fold                      one launch per level from the top down, a gather from the single parent; then the add.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_mesh.h"
#include "../../include/gd_sample.h"
#include "raster_common.h"

namespace gd {
namespace {

constexpr int kThreads = 256;
constexpr int kTexel = GD_SAMPLE_TEXEL;
constexpr float kIndexLimit = 1073741824.0f;   // 2^30

int sfail(const char* what, const char* msg)
{
    char buf[200];
    snprintf(buf, sizeof(buf), "sample %s: %s", what, msg);
    return mesh_fail(-1, buf);
}

dim3 grid_of(int64_t n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }   // false for NaN

// ---- rast_db and the attribute derivatives --------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void rast_db_kernel(int V, int F, int H, int W, const float4* __restrict__ rast,
                                                           const float4* __restrict__ pos, const int* __restrict__ tri,
                                                           float4* __restrict__ rast_db)
{
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= (int64_t)H * W) return;
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float idf = rast[p].w;
    const int t = idf >= 1.0f && idf <= (float)F ? (int)idf - 1 : -1;
    if (t >= 0) {
        const int i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
        if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
            const int r = (int)(p / W), c = (int)(p % W);
            const float4 P0 = pos[i0], P1 = pos[i1], P2 = pos[i2];
            const float fx = (float)(2 * c + 1) / (float)W - 1.0f, fy = (float)(2 * r + 1) / (float)H - 1.0f;
            const float qx0 = P0.x - fx * P0.w, qy0 = P0.y - fy * P0.w;
            const float qx1 = P1.x - fx * P1.w, qy1 = P1.y - fy * P1.w;
            const float qx2 = P2.x - fx * P2.w, qy2 = P2.y - fy * P2.w;
            const float w0 = P0.w, w1 = P1.w, w2 = P2.w;
            const float a0 = qx1 * qy2 - qy1 * qx2;
            const float a1 = qx2 * qy0 - qy2 * qx0;
            const float a2 = qx0 * qy1 - qy0 * qx1;
            const float s = (a0 + a1) + a2;
            if (s != 0.0f && finite_f(s)) {
                const float da0x = qy1 * w2 - w1 * qy2, da1x = qy2 * w0 - w2 * qy0, da2x = qy0 * w1 - w0 * qy1;
                const float da0y = w1 * qx2 - qx1 * w2, da1y = w2 * qx0 - qx2 * w0, da2y = w0 * qx1 - qx0 * w1;
                const float dsx = (da0x + da1x) + da2x, dsy = (da0y + da1y) + da2y;
                const float ss = s * s;
                const float ux = (da0x * s - a0 * dsx) / ss, uy = (da0y * s - a0 * dsy) / ss;
                const float vx = (da1x * s - a1 * dsx) / ss, vy = (da1y * s - a1 * dsy) / ss;
                const float kx = 2.0f / (float)W, ky = 2.0f / (float)H;
                out = make_float4(ux * kx, uy * ky, vx * kx, vy * ky);
            }
        }
    }
    rast_db[p] = out;
}

__global__ __launch_bounds__(kThreads) void interpolate_da_kernel(int V, int F, int C, int64_t npix,
                                                                  const float* __restrict__ attr,
                                                                  const float4* __restrict__ rast,
                                                                  const float4* __restrict__ rast_db,
                                                                  const int* __restrict__ tri, float* __restrict__ out_da)
{
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= npix) return;
    const float idf = rast[p].w;
    const int t = idf >= 1.0f && idf <= (float)F ? (int)idf - 1 : -1;
    bool ok = false;
    int i0 = 0, i1 = 0, i2 = 0;
    if (t >= 0) {
        i0 = tri[3 * (size_t)t];
        i1 = tri[3 * (size_t)t + 1];
        i2 = tri[3 * (size_t)t + 2];
        ok = (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
    }
    const float4 db = rast_db[p];
    float* o = out_da + (size_t)p * 2 * C;
    for (int k = 0; k < C; k++) {
        float dx = 0.0f, dy = 0.0f;
        if (ok) {
            const float a2 = attr[(size_t)i2 * C + k];
            const float e0 = attr[(size_t)i0 * C + k] - a2, e1 = attr[(size_t)i1 * C + k] - a2;
            dx = db.x * e0 + db.z * e1;
            dy = db.y * e0 + db.w * e1;
        }
        o[2 * k] = dx;
        o[2 * k + 1] = dy;
    }
}

// ---- the pyramid ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void pack_level0_kernel(int64_t n, int C, const float* __restrict__ tex,
                                                               float4* __restrict__ pyr)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    float t[kTexel] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < C; k++) t[k] = tex[i * C + k];
    pyr[i] = make_float4(t[0], t[1], t[2], t[3]);
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 scale4(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }

// level (Wc, Hc) from its parent level (Wp, Hp)
__global__ __launch_bounds__(kThreads) void mip_level_kernel(int Wp, int Hp, int Wc, int Hc, const float4* __restrict__ parent,
                                                             float4* __restrict__ child)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)Wc * Hc) return;
    const int x = (int)(i % Wc), y = (int)(i / Wc);
    float4 out;
    if (Wp > 1 && Hp > 1) {
        const float4* row0 = parent + (size_t)(2 * y) * Wp + 2 * x;
        const float4* row1 = row0 + Wp;
        out = scale4(add4(add4(row0[0], row0[1]), add4(row1[0], row1[1])), 0.25f);
    } else if (Wp == 1) {
        out = scale4(add4(parent[2 * y], parent[2 * y + 1]), 0.5f);
    } else {
        out = scale4(add4(parent[2 * x], parent[2 * x + 1]), 0.5f);
    }
    child[i] = out;
}

// ---- sampling -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int tex_index(float i, int n, int boundary)
{
    const int k = (int)fminf(fmaxf(i, -kIndexLimit), kIndexLimit);
    if (boundary == GD_SAMPLE_CLAMP) return min(max(k, 0), n - 1);
    const int m = k % n;
    return m < 0 ? m + n : m;
}

// the four taps of one level: texel indices in the pyramid buffer and the two fractions
struct Taps {
    int idx[4];   // 00, 10, 01, 11
    float fx, fy;
};

__device__ __forceinline__ Taps bilinear_taps(const gd_sample_pyramid& L, int l, float u, float v, int boundary)
{
    const int Wl = L.width[l], Hl = L.height[l];
    const float xs = u * (float)Wl, ys = v * (float)Hl;
    const float x0 = floorf(xs - 0.5f), y0 = floorf(ys - 0.5f);
    Taps t;
    t.fx = (xs - x0) - 0.5f;   // exact for a power-of-two side: xs is, and xs - x0 lies in [0.5, 1.5)
    t.fy = (ys - y0) - 0.5f;
    const int c0 = tex_index(x0, Wl, boundary), c1 = tex_index(x0 + 1.0f, Wl, boundary);
    const int r0 = tex_index(y0, Hl, boundary), r1 = tex_index(y0 + 1.0f, Hl, boundary);
    const int base = L.offset[l];
    t.idx[0] = base + r0 * Wl + c0;
    t.idx[1] = base + r0 * Wl + c1;
    t.idx[2] = base + r1 * Wl + c0;
    t.idx[3] = base + r1 * Wl + c1;
    return t;
}

__device__ __forceinline__ float lerp1(float a, float b, float f) { return a + f * (b - a); }

__device__ __forceinline__ float4 blend(const float4 t[4], float fx, float fy)
{
    float4 o;
    {
        const float p = lerp1(t[0].x, t[1].x, fx), q = lerp1(t[2].x, t[3].x, fx);
        o.x = lerp1(p, q, fy);
    }
    {
        const float p = lerp1(t[0].y, t[1].y, fx), q = lerp1(t[2].y, t[3].y, fx);
        o.y = lerp1(p, q, fy);
    }
    {
        const float p = lerp1(t[0].z, t[1].z, fx), q = lerp1(t[2].z, t[3].z, fx);
        o.z = lerp1(p, q, fy);
    }
    {
        const float p = lerp1(t[0].w, t[1].w, fx), q = lerp1(t[2].w, t[3].w, fx);
        o.w = lerp1(p, q, fy);
    }
    return o;
}

__device__ __forceinline__ float mip_level(const gd_sample_pyramid& L, float4 da)
{
    const float Wt = (float)L.width[0], Ht = (float)L.height[0];
    const float sx = da.x * Wt, sy = da.y * Wt, tx = da.z * Ht, ty = da.w * Ht;
    const float A = sx * sx + tx * tx, B = sy * sy + ty * ty, Cc = sx * sy + tx * ty, d = A - B;
    const float m = 0.5f * (A + B) + sqrtf(0.25f * (d * d) + Cc * Cc);
    if (!(m > 0.0f) || !finite_f(m)) return 0.0f;
    return fminf(fmaxf(0.5f * log2f(m), 0.0f), (float)(L.levels - 1));
}

// The levels and the blend factor of a pixel: l0, l1 and f (f == 0: one level).
__device__ __forceinline__ void pick_levels(const gd_sample_pyramid& L, int filter, const float4* __restrict__ uv_da, int64_t n,
                                            int& l0, int& l1, float& f)
{
    l0 = l1 = 0;
    f = 0.0f;
    if (filter < GD_SAMPLE_LINEAR_MIPMAP_NEAREST) return;
    const float level = mip_level(L, uv_da[n]);
    if (filter == GD_SAMPLE_LINEAR_MIPMAP_NEAREST) {
        l0 = l1 = (int)floorf(level + 0.5f);
        return;
    }
    const float fl = floorf(level);
    l0 = (int)fl;
    f = level - fl;
    l1 = min(l0 + 1, L.levels - 1);
}

__device__ __forceinline__ void store_channels(float* __restrict__ out, int64_t n, int C, float4 o)
{
    float* p = out + n * C;
    p[0] = o.x;
    if (C > 1) p[1] = o.y;
    if (C > 2) p[2] = o.z;
    if (C > 3) p[3] = o.w;
}

template <int FILTER>
__global__ __launch_bounds__(kThreads) void texture_forward_kernel(int N, int C, int boundary, gd_sample_pyramid L,
                                                                   const float4* __restrict__ pyr,
                                                                   const float2* __restrict__ uv,
                                                                   const float4* __restrict__ uv_da, float* __restrict__ out)
{
    const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const float2 p = uv[n];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (finite_f(p.x) && finite_f(p.y)) {
        if (FILTER == GD_SAMPLE_NEAREST) {
            const int Wt = L.width[0], Ht = L.height[0];
            const int ix = tex_index(floorf(p.x * (float)Wt), Wt, boundary);
            const int iy = tex_index(floorf(p.y * (float)Ht), Ht, boundary);
            o = pyr[(size_t)iy * Wt + ix];
        } else {
            int l0, l1;
            float f;
            pick_levels(L, FILTER, uv_da, n, l0, l1, f);
            const Taps a = bilinear_taps(L, l0, p.x, p.y, boundary);
            float4 ta[4];
#pragma unroll
            for (int j = 0; j < 4; j++) ta[j] = pyr[a.idx[j]];
            if (FILTER == GD_SAMPLE_LINEAR_MIPMAP_LINEAR && f != 0.0f) {
                const Taps b = bilinear_taps(L, l1, p.x, p.y, boundary);
                float4 tb[4];
#pragma unroll
                for (int j = 0; j < 4; j++) tb[j] = pyr[b.idx[j]];          // issued before ta is used
                const float4 c0 = blend(ta, a.fx, a.fy), c1 = blend(tb, b.fx, b.fy);
                o = make_float4(lerp1(c0.x, c1.x, f), lerp1(c0.y, c1.y, f), lerp1(c0.z, c1.z, f), lerp1(c0.w, c1.w, f));
            } else {
                o = blend(ta, a.fx, a.fy);
            }
        }
    }
    store_channels(out, n, C, o);
}

// ---- gradient to the texture ----------------------------------------------------------------------------------------
__device__ __forceinline__ void put_item(int64_t* __restrict__ keys, float* __restrict__ vals, int64_t item, int C, int64_t key,
                                         float w, const float* d, bool plain)
{
    keys[item] = key;
    for (int k = 0; k < C; k++) vals[item * C + k] = plain ? d[k] : w * d[k];
}

__device__ __forceinline__ void put_level(int64_t* __restrict__ keys, float* __restrict__ vals, int64_t first, int C,
                                          const Taps& t, float lw, bool scaled, const float* d)
{
    const float gx = 1.0f - t.fx, gy = 1.0f - t.fy;
    const float w[4] = {gx * gy, t.fx * gy, gx * t.fy, t.fx * t.fy};
#pragma unroll
    for (int j = 0; j < 4; j++) put_item(keys, vals, first + j, C, t.idx[j], scaled ? lw * w[j] : w[j], d, false);
}

__global__ __launch_bounds__(kThreads) void texture_items_kernel(int N, int C, int filter, int boundary, int T,
                                                                 gd_sample_pyramid L, const float2* __restrict__ uv,
                                                                 const float4* __restrict__ uv_da,
                                                                 const float* __restrict__ dout, int64_t* __restrict__ keys,
                                                                 float* __restrict__ vals)
{
    const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (n >= N) return;
    const int64_t last = L.offset[L.levels], first = n * T;
    const float2 p = uv[n];
    float d[GD_SAMPLE_MAX_CHANNELS] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = 0; k < C; k++) d[k] = dout[n * C + k];
    const float zero[GD_SAMPLE_MAX_CHANNELS] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (!(finite_f(p.x) && finite_f(p.y))) {
        for (int j = 0; j < T; j++) put_item(keys, vals, first + j, C, last, 0.0f, zero, true);
        return;
    }
    if (filter == GD_SAMPLE_NEAREST) {
        const int Wt = L.width[0], Ht = L.height[0];
        const int ix = tex_index(floorf(p.x * (float)Wt), Wt, boundary);
        const int iy = tex_index(floorf(p.y * (float)Ht), Ht, boundary);
        put_item(keys, vals, first, C, (int64_t)iy * Wt + ix, 1.0f, d, true);
        return;
    }
    int l0, l1;
    float f;
    pick_levels(L, filter, uv_da, n, l0, l1, f);
    const bool two = filter == GD_SAMPLE_LINEAR_MIPMAP_LINEAR && f != 0.0f;
    put_level(keys, vals, first, C, bilinear_taps(L, l0, p.x, p.y, boundary), 1.0f - f, two, d);
    if (T == 8) {
        if (two) put_level(keys, vals, first + 4, C, bilinear_taps(L, l1, p.x, p.y, boundary), f, true, d);
        else
            for (int j = 4; j < 8; j++) put_item(keys, vals, first + j, C, last, 0.0f, zero, true);
    }
}

__global__ __launch_bounds__(kThreads) void texture_reduce_kernel(int64_t items, int C, int64_t total,
                                                                  const int64_t* __restrict__ skeys,
                                                                  const int64_t* __restrict__ order,
                                                                  const float* __restrict__ vals, float* __restrict__ gpyr)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= items) return;
    const int64_t key = skeys[i];
    if (key < 0 || key >= total) return;
    if (i > 0 && skeys[i - 1] == key) return;
    float sum[GD_SAMPLE_MAX_CHANNELS] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t j = i; j < items && skeys[j] == key; j++) {
        const int64_t item = order[j];
        if (item < 0 || item >= items) continue;
        for (int k = 0; k < C; k++) sum[k] += vals[item * C + k];
    }
    for (int k = 0; k < C; k++) gpyr[key * kTexel + k] = sum[k];
}

// g_l += w g_{l+1}[parent]
__global__ __launch_bounds__(kThreads) void fold_level_kernel(int Wl, int Hl, int Wp, float w, float4* __restrict__ fine,
                                                              const float4* __restrict__ coarse)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)Wl * Hl) return;
    const int x = (int)(i % Wl), y = (int)(i / Wl);
    const float4 g = fine[i], c = coarse[(size_t)(y >> 1) * Wp + (x >> 1)];
    fine[i] = make_float4(g.x + w * c.x, g.y + w * c.y, g.z + w * c.z, g.w + w * c.w);
}

__global__ __launch_bounds__(kThreads) void add_level0_kernel(int64_t n, int C, const float* __restrict__ g0,
                                                              float* __restrict__ dtex)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < C; k++) {
        const float g = g0[i * kTexel + k];
        if (g != 0.0f) dtex[i * C + k] = dtex[i * C + k] + g;
    }
}

// ---- argument checks ------------------------------------------------------------------------------------------------
bool pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

int check_layout(const char* what, const gd_sample_pyramid& L)
{
    if (L.levels < 1 || L.levels > GD_SAMPLE_MAX_LEVELS) return sfail(what, "the pyramid must have 1..15 levels");
    gd_sample_pyramid want;
    if (int r = gd_sample_pyramid_layout(L.height[0], L.width[0], L.levels - 1, &want)) return r;
    if (want.levels != L.levels) return sfail(what, "the pyramid has more levels than its sides allow");
    for (int l = 0; l < L.levels; l++)
        if (want.width[l] != L.width[l] || want.height[l] != L.height[l] || want.offset[l] != L.offset[l])
            return sfail(what, "the pyramid is not one of gd_sample_pyramid_layout");
    if (want.offset[L.levels] != L.offset[L.levels]) return sfail(what, "the pyramid is not one of gd_sample_pyramid_layout");
    return 0;
}

int check_sampling(const char* what, int N, int C, int filter, int boundary, const gd_sample_pyramid& L, const void* uv_da)
{
    if (C < 1 || C > GD_SAMPLE_MAX_CHANNELS) return sfail(what, "C must be in 1..4");
    const int T = gd_sample_taps(filter);
    if (T < 0) return sfail(what, "unknown filter mode");
    if (boundary != GD_SAMPLE_WRAP && boundary != GD_SAMPLE_CLAMP) return sfail(what, "unknown boundary mode");
    if (N < 1 || (int64_t)N * T >= ((int64_t)1 << 31)) return sfail(what, "N must be at least 1 and N taps below 2^31");
    if (int r = check_layout(what, L)) return r;
    if (filter >= GD_SAMPLE_LINEAR_MIPMAP_NEAREST) {
        if (!uv_da) return sfail(what, "a mip filter needs uv_da");
        if (!pow2(L.width[0]) || !pow2(L.height[0])) return sfail(what, "a mip filter needs power-of-two sides");
    }
    return 0;
}

int check_image(const char* what, int V, int F, int H, int W)
{
    if (V < 1 || F < 1 || F >= (1 << 24)) return sfail(what, "V must be at least 1 and F in 1..2^24-1");
    if (H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 29)) return sfail(what, "H and W must be at least 1 and H W below 2^29");
    return 0;
}

}  // namespace
}  // namespace gd

extern "C" {

using namespace gd;

int gd_sample_taps(int filter)
{
    switch (filter) {
        case GD_SAMPLE_NEAREST: return 1;
        case GD_SAMPLE_LINEAR: return 4;
        case GD_SAMPLE_LINEAR_MIPMAP_NEAREST: return 4;
        case GD_SAMPLE_LINEAR_MIPMAP_LINEAR: return 8;
        default: return -1;
    }
}

int gd_sample_pyramid_layout(int Ht, int Wt, int max_mip_level, gd_sample_pyramid* out)
{
    const char* what = "pyramid layout";
    if (!out) return sfail(what, "null pointer");
    if (Ht < 1 || Wt < 1 || Ht > GD_SAMPLE_MAX_SIDE || Wt > GD_SAMPLE_MAX_SIDE) return sfail(what, "the sides must be in 1..16384");
    int full = 0;
    while ((max(Wt, Ht) >> (full + 1)) > 0) full++;
    const int top = max_mip_level < 0 ? full : min(max_mip_level, full);
    if (top > 0 && (!pow2(Wt) || !pow2(Ht))) return sfail(what, "mip levels need power-of-two sides");
    gd_sample_pyramid L = {};
    L.levels = top + 1;
    int64_t at = 0;
    for (int l = 0; l <= top; l++) {
        L.width[l] = max(Wt >> l, 1);
        L.height[l] = max(Ht >> l, 1);
        L.offset[l] = (int32_t)at;
        at += (int64_t)L.width[l] * L.height[l];
    }
    L.offset[top + 1] = (int32_t)at;
    *out = L;
    return 0;
}

int gd_sample_rast_db(void* stream, int V, int F, int H, int W, const float* rast, const float* pos, const int* tri,
                      float* rast_db)
{
    const char* what = "rast_db";
    if (!rast || !pos || !tri || !rast_db) return sfail(what, "null pointer");
    if (int r = check_image(what, V, F, H, W)) return r;
    hipLaunchKernelGGL(rast_db_kernel, grid_of((int64_t)H * W), dim3(kThreads), 0, (hipStream_t)stream, V, F, H, W,
                       reinterpret_cast<const float4*>(rast), reinterpret_cast<const float4*>(pos), tri,
                       reinterpret_cast<float4*>(rast_db));
    return mesh_launched("sample", what);
}

int gd_sample_interpolate_da(void* stream, int V, int F, int C, int H, int W, const float* attr, const float* rast,
                             const float* rast_db, const int* tri, float* out_da)
{
    const char* what = "interpolate_da";
    if (!attr || !rast || !rast_db || !tri || !out_da) return sfail(what, "null pointer");
    if (int r = check_image(what, V, F, H, W)) return r;
    if (C < 1 || C > GD_MESH_MAX_CHANNELS) return sfail(what, "C must be in 1..8");
    hipLaunchKernelGGL(interpolate_da_kernel, grid_of((int64_t)H * W), dim3(kThreads), 0, (hipStream_t)stream, V, F, C,
                       (int64_t)H * W, attr, reinterpret_cast<const float4*>(rast), reinterpret_cast<const float4*>(rast_db),
                       tri, out_da);
    return mesh_launched("sample", what);
}

int gd_sample_build_mips(void* stream, int C, const float* tex, gd_sample_pyramid L, float* pyr)
{
    const char* what = "build mips";
    if (!tex || !pyr) return sfail(what, "null pointer");
    if (C < 1 || C > GD_SAMPLE_MAX_CHANNELS) return sfail(what, "C must be in 1..4");
    if (int r = check_layout(what, L)) return r;
    hipStream_t s = (hipStream_t)stream;
    float4* p = reinterpret_cast<float4*>(pyr);
    const int64_t n0 = (int64_t)L.width[0] * L.height[0];
    hipLaunchKernelGGL(pack_level0_kernel, grid_of(n0), dim3(kThreads), 0, s, n0, C, tex, p);
    for (int l = 1; l < L.levels; l++)
        hipLaunchKernelGGL(mip_level_kernel, grid_of((int64_t)L.width[l] * L.height[l]), dim3(kThreads), 0, s, L.width[l - 1],
                           L.height[l - 1], L.width[l], L.height[l], p + L.offset[l - 1], p + L.offset[l]);
    return mesh_launched("sample", what);
}

int gd_sample_texture_forward(void* stream, int N, int C, int filter, int boundary, gd_sample_pyramid L, const float* pyr,
                              const float* uv, const float* uv_da, float* out)
{
    const char* what = "texture forward";
    if (!pyr || !uv || !out) return sfail(what, "null pointer");
    if (int r = check_sampling(what, N, C, filter, boundary, L, uv_da)) return r;
    hipStream_t s = (hipStream_t)stream;
    const float4* p = reinterpret_cast<const float4*>(pyr);
    const float2* q = reinterpret_cast<const float2*>(uv);
    const float4* da = reinterpret_cast<const float4*>(uv_da);
    const dim3 grid = grid_of(N), block(kThreads);
    switch (filter) {
        case GD_SAMPLE_NEAREST:
            hipLaunchKernelGGL(texture_forward_kernel<GD_SAMPLE_NEAREST>, grid, block, 0, s, N, C, boundary, L, p, q, da, out);
            break;
        case GD_SAMPLE_LINEAR:
            hipLaunchKernelGGL(texture_forward_kernel<GD_SAMPLE_LINEAR>, grid, block, 0, s, N, C, boundary, L, p, q, da, out);
            break;
        case GD_SAMPLE_LINEAR_MIPMAP_NEAREST:
            hipLaunchKernelGGL(texture_forward_kernel<GD_SAMPLE_LINEAR_MIPMAP_NEAREST>, grid, block, 0, s, N, C, boundary, L, p,
                               q, da, out);
            break;
        default:
            hipLaunchKernelGGL(texture_forward_kernel<GD_SAMPLE_LINEAR_MIPMAP_LINEAR>, grid, block, 0, s, N, C, boundary, L, p,
                               q, da, out);
            break;
    }
    return mesh_launched("sample", what);
}

int gd_sample_texture_items(void* stream, int N, int C, int filter, int boundary, gd_sample_pyramid L, const float* uv,
                            const float* uv_da, const float* dout, int64_t* keys, float* vals)
{
    const char* what = "texture items";
    if (!uv || !dout || !keys || !vals) return sfail(what, "null pointer");
    if (int r = check_sampling(what, N, C, filter, boundary, L, uv_da)) return r;
    hipLaunchKernelGGL(texture_items_kernel, grid_of(N), dim3(kThreads), 0, (hipStream_t)stream, N, C, filter, boundary,
                       gd_sample_taps(filter), L, reinterpret_cast<const float2*>(uv), reinterpret_cast<const float4*>(uv_da),
                       dout, keys, vals);
    return mesh_launched("sample", what);
}

int gd_sample_texture_reduce(void* stream, int64_t items, int C, gd_sample_pyramid L, const int64_t* sorted_keys,
                             const int64_t* order, const float* vals, float* gpyr)
{
    const char* what = "texture reduce";
    if (!sorted_keys || !order || !vals || !gpyr) return sfail(what, "null pointer");
    if (C < 1 || C > GD_SAMPLE_MAX_CHANNELS) return sfail(what, "C must be in 1..4");
    if (items < 1 || items >= ((int64_t)1 << 31)) return sfail(what, "items must be in 1..2^31-1");
    if (int r = check_layout(what, L)) return r;
    hipLaunchKernelGGL(texture_reduce_kernel, grid_of(items), dim3(kThreads), 0, (hipStream_t)stream, items, C,
                       (int64_t)L.offset[L.levels], sorted_keys, order, vals, gpyr);
    return mesh_launched("sample", what);
}

int gd_sample_texture_fold(void* stream, int C, gd_sample_pyramid L, float* gpyr, float* dtex)
{
    const char* what = "texture fold";
    if (!gpyr || !dtex) return sfail(what, "null pointer");
    if (C < 1 || C > GD_SAMPLE_MAX_CHANNELS) return sfail(what, "C must be in 1..4");
    if (int r = check_layout(what, L)) return r;
    hipStream_t s = (hipStream_t)stream;
    float4* g = reinterpret_cast<float4*>(gpyr);
    for (int l = L.levels - 2; l >= 0; l--) {
        const int Wl = L.width[l], Hl = L.height[l];
        hipLaunchKernelGGL(fold_level_kernel, grid_of((int64_t)Wl * Hl), dim3(kThreads), 0, s, Wl, Hl, L.width[l + 1],
                           (Wl > 1 && Hl > 1) ? 0.25f : 0.5f, g + L.offset[l], g + L.offset[l + 1]);
    }
    const int64_t n0 = (int64_t)L.width[0] * L.height[0];
    hipLaunchKernelGGL(add_level0_kernel, grid_of(n0), dim3(kThreads), 0, s, n0, C, gpyr, dtex);
    return mesh_launched("sample", what);
}

}  // extern "C"
