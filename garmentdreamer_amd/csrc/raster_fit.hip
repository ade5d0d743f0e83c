// raster_fit.hip -- the loss head of the NeTF stage's texture fit (C-ABI and the DEFINITIONS: include/gd_fit.h): the tail
// of Renderer.render (clamp, composite, view cosine) and the masked MSE of Renderer.fit_texture_from_mesh against one
// captured view, forward and backward.  Built with -ffp-contract=off: the header fixes the order of every operation.
//
// Streaming passes over 1024 x 1024 images: 73 bytes per pixel forward (56 read, 17 written), 41 backward, against some 170
// VALU instructions per pixel forward (three IEEE divisions for the normalisation, one for the cosine, three square
// roots).  A lane takes FOUR consecutive pixels, so that every [.,3] image is three 16-byte loads per lane and every [.]
// image one (a lane per pixel reads 4-byte words 12 bytes apart); a wave is 256 pixels = one partial of the header.  The
// wide path needs the quad inside the image, and for the targets under flip_rows a width that is a multiple of 4 (the
// flipped row then starts on a 16-byte boundary); the quad that does not qualify falls back to scalar loads.
//   forward    fit_pixel_kernel (256 threads = 4 partials; a 64-lane LDS tree per wave) -> fit_final_kernel (one workgroup)
//   backward   fit_backward_kernel (recomputes image, reads m, count and dloss from device memory)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_fit.h"
#include "raster_common.h"

namespace gd {
namespace {

constexpr float kNormEps = 1e-12f;    // torch.nn.functional.normalize
constexpr float kViewEps = 1e-6f;     // the eps the reference passes to cosine_similarity
constexpr int kLane = GD_FIT_PIXELS_PER_LANE;
constexpr int kBlock = 256;
constexpr int kBlockPixels = kBlock * kLane;
static_assert(kLane == 4 && GD_FIT_PIXELS_PER_PARTIAL == 64 * kLane, "a wave is one partial, a lane one float4");
static_assert(GD_FIT_FINAL_THREADS == 256, "fit_final_kernel's tree");

__device__ __forceinline__ float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }

// the C floats of pixels base ... base + n - 1 (0 beyond): C / 4 ... 16-byte loads if wide, else scalar
template <int C>
__device__ __forceinline__ void load_quad(const float* __restrict__ p, size_t base, int n, bool wide, float (&out)[kLane * C])
{
    if (wide) {
        const float4* q = reinterpret_cast<const float4*>(p + C * base);
#pragma unroll
        for (int k = 0; k < C; k++) {
            const float4 v = q[k];
            out[4 * k] = v.x, out[4 * k + 1] = v.y, out[4 * k + 2] = v.z, out[4 * k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kLane * C; k++) out[k] = k < C * n ? p[C * base + k] : 0.0f;
    }
}

template <int C>
__device__ __forceinline__ void store_quad(float* __restrict__ p, size_t base, int n, const float (&in)[kLane * C])
{
    if (n == kLane) {
        float4* q = reinterpret_cast<float4*>(p + C * base);
#pragma unroll
        for (int k = 0; k < C; k++) q[k] = make_float4(in[4 * k], in[4 * k + 1], in[4 * k + 2], in[4 * k + 3]);
    } else {
        for (int k = 0; k < C * n; k++) p[C * base + k] = in[k];
    }
}

// the targets of a quad: pixel j of it reads target pixel at[j]
struct Targets {
    float rgb[kLane * 3], tmask[kLane];
};

__device__ __forceinline__ Targets load_targets(const float* __restrict__ rgb, const float* __restrict__ tmask, int H, int W,
                                                bool flip, size_t base, int n, bool want_mask)
{
    Targets t;
    if (!flip || (n == kLane && W % kLane == 0)) {      // one run of pixels: the quad lies in one row, or nothing is flipped
        size_t at = base;
        if (flip) {
            const size_t y = base / (size_t)W;
            at = ((size_t)H - 1 - y) * (size_t)W + (base - y * (size_t)W);
        }
        load_quad<3>(rgb, at, n, n == kLane, t.rgb);
        if (want_mask) load_quad<1>(tmask, at, n, n == kLane, t.tmask);
        return t;
    }
    size_t y = base / (size_t)W, x = base - y * (size_t)W;
#pragma unroll
    for (int j = 0; j < kLane; j++) {
        t.rgb[3 * j] = t.rgb[3 * j + 1] = t.rgb[3 * j + 2] = t.tmask[j] = 0.0f;
        if (j < n) {
            const size_t at = ((size_t)H - 1 - y) * (size_t)W + x;
            t.rgb[3 * j] = rgb[3 * at], t.rgb[3 * j + 1] = rgb[3 * at + 1], t.rgb[3 * j + 2] = rgb[3 * at + 2];
            if (want_mask) t.tmask[j] = tmask[at];
        }
        if (++x == (size_t)W) x = 0, y++;
    }
    return t;
}

// image_k = a c_k + (1 - a) bg_k of one pixel, the header's four roundings
__device__ __forceinline__ void composite(float a, const float* c_aa, const float* bg, float* image)
{
    const float u = 1.0f - a;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float s = a * clamp01(c_aa[k]);
        const float t = u * bg[k];
        image[k] = s + t;
    }
}

// scratch: float sums[partials], then int32 counts[partials]
__global__ __launch_bounds__(kBlock) void fit_pixel_kernel(size_t npix, int H, int W, int flip, size_t partials,
                                                           const float* __restrict__ c_aa, const float* __restrict__ a_aa,
                                                           const float* __restrict__ p_aa, const float* __restrict__ n_aa,
                                                           const float* __restrict__ center, const float* __restrict__ rgb,
                                                           const float* __restrict__ tmask, const float* __restrict__ bg,
                                                           float* __restrict__ image, float* __restrict__ cosinesview,
                                                           uint8_t* __restrict__ m, float* __restrict__ scratch)
{
    __shared__ float lds_f[kBlock];
    __shared__ int lds_i[kBlock];
    const int t = threadIdx.x, lane = t & 63;
    const size_t base = ((size_t)blockIdx.x * kBlock + t) * kLane;
    float q = 0.0f;
    int count = 0;
    if (base < npix) {
        const int n = npix - base < (size_t)kLane ? (int)(npix - base) : kLane;
        const bool wide = n == kLane;
        float c[12], a[4], p[12], nrm[12], img[12], cs[4];
        load_quad<3>(c_aa, base, n, wide, c);
        load_quad<1>(a_aa, base, n, wide, a);
        load_quad<3>(p_aa, base, n, wide, p);
        load_quad<3>(n_aa, base, n, wide, nrm);
        const Targets tg = load_targets(rgb, tmask, H, W, flip != 0, base, n, true);
        const float ctr[3] = {center[0], center[1], center[2]};
        const float bgc[3] = {bg[0], bg[1], bg[2]};
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < kLane; j++) {
            const float aj = clamp01(a[j]);
            composite(aj, c + 3 * j, bgc, img + 3 * j);
            float d[3] = {p[3 * j] - ctr[0], p[3 * j + 1] - ctr[1], p[3 * j + 2] - ctr[2]};
            const float len = fmaxf(sqrtf(dot3(d, d)), kNormEps);
            d[0] = d[0] / len, d[1] = d[1] / len, d[2] = d[2] / len;
            const float* nj = nrm + 3 * j;
            cs[j] = dot3(d, nj) / (fmaxf(sqrtf(dot3(d, d)), kViewEps) * fmaxf(sqrtf(dot3(nj, nj)), kViewEps));
            const bool in = j < n && aj > 0.0f && tg.tmask[j] > 0.0f && cs[j] <= 0.0f;
            const float r[3] = {img[3 * j] - tg.rgb[3 * j], img[3 * j + 1] - tg.rgb[3 * j + 1],
                                img[3 * j + 2] - tg.rgb[3 * j + 2]};
            const float e = in ? dot3(r, r) : 0.0f;
            q = j == 0 ? e : q + e;
            count += in;
            packed |= (uint32_t)in << (8 * j);
        }
        store_quad<3>(image, base, n, img);
        store_quad<1>(cosinesview, base, n, cs);
        if (wide)
            *reinterpret_cast<uint32_t*>(m + base) = packed;
        else
            for (int j = 0; j < n; j++) m[base + j] = (uint8_t)(packed >> (8 * j) & 1);
    }
    lds_f[t] = q;
    lds_i[t] = count;
    __syncthreads();
#pragma unroll
    for (int stride = 32; stride > 0; stride >>= 1) {
        if (lane < stride) {
            lds_f[t] += lds_f[t + stride];
            lds_i[t] += lds_i[t + stride];
        }
        __syncthreads();
    }
    const size_t partial = (size_t)blockIdx.x * (kBlock / 64) + (t >> 6);
    if (lane == 0 && partial < partials) {
        scratch[partial] = lds_f[t];
        reinterpret_cast<int*>(scratch)[partials + partial] = lds_i[t];
    }
}

__global__ __launch_bounds__(GD_FIT_FINAL_THREADS) void fit_final_kernel(size_t partials, const float* __restrict__ scratch,
                                                                         float* __restrict__ stats)
{
    __shared__ float lds_f[GD_FIT_FINAL_THREADS];
    __shared__ int lds_i[GD_FIT_FINAL_THREADS];
    const int t = threadIdx.x;
    const int* counts = reinterpret_cast<const int*>(scratch) + partials;
    float x = 0.0f;
    int c = 0;
    for (size_t b = t; b < partials; b += GD_FIT_FINAL_THREADS) {
        x += scratch[b];
        c += counts[b];
    }
    lds_f[t] = x;
    lds_i[t] = c;
    __syncthreads();
#pragma unroll
    for (int stride = GD_FIT_FINAL_THREADS / 2; stride > 0; stride >>= 1) {
        if (t < stride) {
            lds_f[t] += lds_f[t + stride];
            lds_i[t] += lds_i[t + stride];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float sum = lds_f[0];
        const int count = lds_i[0];
        stats[0] = count > 0 ? sum / (3.0f * (float)count) : 0.0f;
        reinterpret_cast<int*>(stats)[1] = count;
        stats[2] = sum;
        stats[3] = 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void fit_backward_kernel(size_t npix, int H, int W, int flip,
                                                              const float* __restrict__ c_aa, const float* __restrict__ a_aa,
                                                              const float* __restrict__ rgb, const float* __restrict__ bg,
                                                              const uint8_t* __restrict__ m, const float* __restrict__ stats,
                                                              const float* __restrict__ dloss, float* __restrict__ dc_aa)
{
    const size_t base = ((size_t)blockIdx.x * kBlock + threadIdx.x) * kLane;
    if (base >= npix) return;
    const int n = npix - base < (size_t)kLane ? (int)(npix - base) : kLane;
    const bool wide = n == kLane;
    uint32_t packed = 0;
    if (wide)
        packed = *reinterpret_cast<const uint32_t*>(m + base);
    else
        for (int j = 0; j < n; j++) packed |= (uint32_t)(m[base + j] != 0) << (8 * j);
    float dc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) dc[k] = 0.0f;
    const int count = reinterpret_cast<const int*>(stats)[1];
    if (packed != 0 && count > 0) {                      // a quad nothing selected reads nothing more
        const float g = (2.0f * dloss[0]) / (3.0f * (float)count);
        float c[12], a[4], img[3];
        load_quad<3>(c_aa, base, n, wide, c);
        load_quad<1>(a_aa, base, n, wide, a);
        const Targets tg = load_targets(rgb, nullptr, H, W, flip != 0, base, n, false);
        const float bgc[3] = {bg[0], bg[1], bg[2]};
#pragma unroll
        for (int j = 0; j < kLane; j++) {
            if (!(packed >> (8 * j) & 1)) continue;
            const float aj = clamp01(a[j]);
            composite(aj, c + 3 * j, bgc, img);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const float ck = c[3 * j + k];
                if (ck >= 0.0f && ck <= 1.0f) dc[3 * j + k] = (g * (img[k] - tg.rgb[3 * j + k])) * aj;
            }
        }
    }
    store_quad<3>(dc_aa, base, n, dc);
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t partials_of(size_t npix) { return (npix + GD_FIT_PIXELS_PER_PARTIAL - 1) / GD_FIT_PIXELS_PER_PARTIAL; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// -1 with a message, or 0
int validate(const char* what, int H, int W, bool all_present, bool all_aligned)
{
    char buf[200];
    if (H <= 0 || W <= 0 || (int64_t)H * W >= ((int64_t)1 << 30)) {
        snprintf(buf, sizeof(buf), "%s: H and W must be positive and H W < 2^30", what);
        return mesh_fail(-1, buf);
    }
    if (!all_present) {
        snprintf(buf, sizeof(buf), "%s: null pointer", what);
        return mesh_fail(-1, buf);
    }
    if (!all_aligned) {
        snprintf(buf, sizeof(buf), "%s: every image must be 16-byte aligned", what);
        return mesh_fail(-1, buf);
    }
    return 0;
}

}  // namespace
}  // namespace gd

extern "C" {

size_t gd_fit_loss_scratch_bytes(int64_t pixels)
{
    if (pixels <= 0) return 0;
    return gd::align256(gd::partials_of((size_t)pixels) * (sizeof(float) + sizeof(int32_t)));
}

int gd_fit_loss_forward(void* stream, int H, int W, int flip_rows, const float* c_aa, const float* a_aa, const float* p_aa,
                        const float* n_aa, const float* center, const float* rgb, const float* tmask, const float* bg,
                        float* image, float* cosinesview, uint8_t* m, void* stats, void* scratch)
{
    using namespace gd;
    const bool present = c_aa && a_aa && p_aa && n_aa && center && rgb && tmask && bg && image && cosinesview && m && stats
        && scratch;
    const bool aligned = aligned16(c_aa) && aligned16(a_aa) && aligned16(p_aa) && aligned16(n_aa) && aligned16(rgb)
        && aligned16(tmask) && aligned16(image) && aligned16(cosinesview) && aligned16(m) && aligned16(scratch);
    if (validate("fit loss", H, W, present, aligned)) return -1;
    hipStream_t s = (hipStream_t)stream;
    const size_t npix = (size_t)H * W, partials = partials_of(npix);
    const unsigned blocks = (unsigned)((npix + kBlockPixels - 1) / kBlockPixels);
    hipLaunchKernelGGL(fit_pixel_kernel, dim3(blocks), dim3(kBlock), 0, s, npix, H, W, flip_rows, partials, c_aa, a_aa,
                       p_aa, n_aa, center, rgb, tmask, bg, image, cosinesview, m, (float*)scratch);
    hipLaunchKernelGGL(fit_final_kernel, dim3(1), dim3(GD_FIT_FINAL_THREADS), 0, s, partials, (const float*)scratch,
                       (float*)stats);
    return mesh_launched(nullptr, "fit loss forward");
}

int gd_fit_loss_backward(void* stream, int H, int W, int flip_rows, const float* c_aa, const float* a_aa, const float* rgb,
                         const float* bg, const uint8_t* m, const void* stats, const float* dloss, float* dc_aa)
{
    using namespace gd;
    const bool present = c_aa && a_aa && rgb && bg && m && stats && dloss && dc_aa;
    const bool aligned = aligned16(c_aa) && aligned16(a_aa) && aligned16(rgb) && aligned16(m) && aligned16(dc_aa);
    if (validate("fit loss backward", H, W, present, aligned)) return -1;
    const size_t npix = (size_t)H * W;
    hipLaunchKernelGGL(fit_backward_kernel, dim3((unsigned)((npix + kBlockPixels - 1) / kBlockPixels)), dim3(kBlock), 0,
                       (hipStream_t)stream, npix, H, W, flip_rows, c_aa, a_aa, rgb, bg, m, (const float*)stats, dloss, dc_aa);
    return mesh_launched(nullptr, "fit loss backward");
}

}  // extern "C"
