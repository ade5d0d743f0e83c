// raster_views.hip -- reading the captured views (C-ABI and the DEFINITIONS: include/gd_views.h): the row unfilter of
// inflated 8-bit PNG streams and the unpacking of a view's byte images into float images.  Built with -ffp-contract=off:
// the header fixes the order of every fp32 operation; the unfilter is integers only.
//
// UNFILTER.  Pixel (r, x) needs (r, x-1), (r-1, x) and (r-1, x-1): the pixels of an anti-diagonal are independent.  One
// wave owns one image and walks it in BANDS of 64 rows, lane = row of the band: at step s lane l reconstructs pixel
// x = s - l of its row.  a (its own pixel of the step before) stays in a register, b comes from the lane above by a
// cross-lane move of that lane's pixel of the step before, c is the b of the step before.  Lane 0 takes b from the CARRY
// line in LDS, the last row of the band before (zero for the first band).  Bands follow each other inside the wave: no
// workgroup waits on another, there are no atomics, and every loop is bounded by H and W.
//   The filtered bytes go through LDS in CHUNKS of 64 pixels per row, two slots per row used as a ring (pixel x lives at
// x mod 128): a phase of 64 steps starts by flushing chunk m-2 (complete: lane 63 left it at least one step ago, 64 >= 63),
// loading chunk m into the slot that frees, and then runs without touching global memory -- no dependent global load per
// step.  Rows start at byte r (1 + W bpp) + 1 of the stream, so the loads are aligned dwords funnel-shifted into place
// (64 lanes x 4 bytes = the 256 bytes of a 4-byte-pixel chunk); reconstruction overwrites the chunk in place and the flush
// writes rows of it back as 256 contiguous bytes.  With 4-byte pixels lane l reads dword 127 l + s of the tile at step s:
// 64 different banks.
//   LDS: 64 rows x 128 pixels (32 KiB at bpp 4) plus the carry line (W bpp bytes, at most 32 KiB, only when H > 64).
//
// UNPACK.  Bandwidth-bound streaming passes, four pixels per lane: 16-byte loads of the byte images, float4 stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_views.h"
#include "raster_common.h"

namespace gd {
namespace {

constexpr int kBand = GD_VIEWS_BAND_ROWS;
constexpr int kChunk = GD_VIEWS_CHUNK_PIXELS;
constexpr int kRing = 2 * kChunk;       // pixels of a tile row
static_assert(kBand == 64 && kChunk == 64, "one lane per row of a band; a chunk outlasts the skew of the lanes (64 >= 63)");

// The aligned dword at byte offset off (a multiple of 4) of base[0 .. total): bytes past the end read as 0.
__device__ __forceinline__ uint32_t load_dword(const uint8_t* __restrict__ base, size_t total, size_t off)
{
    if (off + 4 <= total) return *reinterpret_cast<const uint32_t*>(base + off);
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (off + k < total) v |= (uint32_t)base[off + k] << (8 * k);
    return v;
}

__device__ __forceinline__ int predict(int type, int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    return type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : type == 4 ? paeth : 0;
}

// one pixel: the bytes of f, a, b, c packed little-endian
template <int BPP>
__device__ __forceinline__ uint32_t reconstruct(int type, uint32_t f, uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < BPP; k++) {
        const int sh = 8 * k;
        const int pred = predict(type, (a >> sh) & 255, (b >> sh) & 255, (c >> sh) & 255);
        out |= ((((f >> sh) & 255) + (uint32_t)pred) & 255u) << sh;
    }
    return out;
}

template <int BPP>
__device__ __forceinline__ uint32_t load_pixel(const uint8_t* p)
{
    if (BPP == 4) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

template <int BPP>
__device__ __forceinline__ void store_pixel(uint8_t* p, uint32_t v)
{
    if (BPP == 4) {
        *reinterpret_cast<uint32_t*>(p) = v;
    } else {
        p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16);
    }
}

// all: bytes of all B streams, the bound of every read of `filtered`
template <int BPP>
__global__ __launch_bounds__(kBand) void png_unfilter_kernel(const uint8_t* __restrict__ filtered, uint8_t* __restrict__ out,
                                                             size_t all, int H, int W, int with_carry)
{
    extern __shared__ uint32_t lds_words[];
    constexpr int kRowBytes = kRing * BPP;         // of a tile row
    constexpr int kChunkBytes = kChunk * BPP;      // a multiple of 4
    constexpr int kChunkWords = kChunkBytes / 4;   // 64 or 48: at most one per lane
    uint8_t* tile = reinterpret_cast<uint8_t*>(lds_words);
    uint8_t* carry = tile + kBand * kRowBytes;     // [nchunks * kChunkBytes], present iff with_carry
    const int lane = threadIdx.x;
    const size_t stride = (size_t)W * BPP, in_row = stride + 1;
    const size_t image = (size_t)blockIdx.x * H * in_row;          // byte offset of this stream in `filtered`
    uint8_t* dst = out + (size_t)blockIdx.x * H * stride;
    const int nchunks = (W + kChunk - 1) / kChunk;
    const int nbands = (H + kBand - 1) / kBand;

    for (int band = 0; band < nbands; band++) {
        const int row0 = band * kBand;
        const int rows = min(kBand, H - row0);                     // of this band
        const int row = row0 + lane;
        const bool has_row = lane < rows;
        int type = 0;
        if (has_row) type = filtered[image + (size_t)row * in_row];    // < all: row < H
        if (type > 4) type = 0;
        uint32_t mine = 0, above_before = 0;                       // recon(r, x-1) and recon(r-1, x-1)

        // chunk mm of the band, complete in its slot, to `out`; the band's last row also to the carry line
        auto flush = [&](int mm) {
            const int slot = mm & 1;
            const int px0 = mm * kChunk;
            const int nbytes = min(kChunk, W - px0) * BPP;
            for (int r = 0; r < rows; r++) {
                const uint8_t* from = tile + r * kRowBytes + slot * kChunkBytes;
                uint8_t* to = dst + (size_t)(row0 + r) * stride + (size_t)px0 * BPP;
                if (BPP == 4) {
                    if (4 * lane < nbytes)
                        reinterpret_cast<uint32_t*>(to)[lane] = reinterpret_cast<const uint32_t*>(from)[lane];
                } else {
                    for (int j = lane; j < nbytes; j += kBand) to[j] = from[j];
                }
            }
            if (with_carry && rows == kBand && lane < kChunkWords)
                reinterpret_cast<uint32_t*>(carry + mm * kChunkBytes)[lane] =
                    reinterpret_cast<const uint32_t*>(tile + (kBand - 1) * kRowBytes + slot * kChunkBytes)[lane];
        };

        // phase m = steps 64 m ... 64 m + 63; the last lane reaches pixel W - 1 at step W + 62 < 64 (nchunks + 1)
        for (int m = 0; m <= nchunks; m++) {
            __syncthreads();
            if (m >= 2) flush(m - 2);
            __syncthreads();
            if (m < nchunks) {
                // load chunk m: per row the dwords that cover its bytes, shifted into place
                const int slot = m & 1;
                const int nbytes = min(kChunk, W - m * kChunk) * BPP;
                const bool takes = lane < kChunkWords && 4 * lane < nbytes;
                for (int r0 = 0; r0 < rows; r0 += 8) {
                    uint32_t v[8];
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        v[k] = 0;
                        if (takes && r0 + k < rows) {
                            const size_t g0 = image + (size_t)(row0 + r0 + k) * in_row + 1 + (size_t)m * kChunkBytes;
                            const size_t ga = (g0 & ~(size_t)3) + 4 * (size_t)lane;
                            const uint32_t shift = 8 * (uint32_t)(g0 & 3);
                            const uint32_t d0 = load_dword(filtered, all, ga);
                            v[k] = d0;
                            if (shift) v[k] = (d0 >> shift) | (load_dword(filtered, all, ga + 4) << (32 - shift));
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 8; k++)
                        if (takes && r0 + k < rows)
                            reinterpret_cast<uint32_t*>(tile + (r0 + k) * kRowBytes + slot * kChunkBytes)[lane] = v[k];
                }
            }
            __syncthreads();
            for (int k = 0; k < kChunk; k++) {
                const int x = m * kChunk + k - lane;
                const bool active = has_row && x >= 0 && x < W;
                uint32_t above = __shfl_up(mine, 1);               // recon(r-1, x): the lane above made it one step ago
                if (lane == 0) above = (band > 0 && active) ? load_pixel<BPP>(carry + (size_t)x * BPP) : 0u;
                if (active) {
                    uint8_t* at = tile + lane * kRowBytes + (x & (kRing - 1)) * BPP;
                    const uint32_t a = x == 0 ? 0u : mine, c = x == 0 ? 0u : above_before;
                    mine = reconstruct<BPP>(type, load_pixel<BPP>(at), a, above, c);
                    store_pixel<BPP>(at, mine);
                    above_before = above;
                }
            }
        }
        __syncthreads();
        flush(nchunks - 1);                                        // chunk nchunks - 2 went out in the last phase
        __syncthreads();
    }
}

// ---- unpack ---------------------------------------------------------------------------------------------------------
constexpr int kLane = GD_VIEWS_PIXELS_PER_LANE;
constexpr int kBlock = 256;
constexpr int kBlockPixels = kBlock * kLane;
static_assert(kLane == 4, "a lane is one uint4 of an RGBA image and one float4 of a mask");

__device__ __forceinline__ float unit(uint32_t byte) { return (float)byte / 255.0f; }

// the C bytes of pixels base ... base + n - 1 (0 beyond); 4-byte loads when the quad is whole
template <int C>
__device__ __forceinline__ void load_bytes(const uint8_t* __restrict__ p, size_t base, int n, uint32_t (&out)[kLane * C])
{
    if (n == kLane) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p + C * base);   // C * base is a multiple of 4
#pragma unroll
        for (int k = 0; k < C; k++) {
            const uint32_t w = q[k];
#pragma unroll
            for (int j = 0; j < 4; j++) out[4 * k + j] = (w >> (8 * j)) & 255u;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kLane * C; k++) out[k] = k < C * n ? (uint32_t)p[C * base + k] : 0u;
    }
}

template <int C>
__device__ __forceinline__ void store_floats(float* __restrict__ p, size_t base, int n, const float (&in)[kLane * C])
{
    if (n == kLane) {
        float4* q = reinterpret_cast<float4*>(p + C * base);
#pragma unroll
        for (int k = 0; k < C; k++) q[k] = make_float4(in[4 * k], in[4 * k + 1], in[4 * k + 2], in[4 * k + 3]);
    } else {
        for (int k = 0; k < C * n; k++) p[C * base + k] = in[k];
    }
}

// kNormal: normal and mask from normal_rgba, rgb_out from rgb [.,C].  Otherwise rgb_out and mask from rgb [.,4].
template <int C, bool kNormal>
__global__ __launch_bounds__(kBlock) void unpack_kernel(size_t npix, const uint8_t* __restrict__ normal_rgba,
                                                        const uint8_t* __restrict__ rgb, float* __restrict__ normal,
                                                        float* __restrict__ mask, float* __restrict__ rgb_out)
{
    const size_t base = ((size_t)blockIdx.x * kBlock + threadIdx.x) * kLane;
    if (base >= npix) return;
    const int n = npix - base < (size_t)kLane ? (int)(npix - base) : kLane;
    uint32_t cb[kLane * C];
    float colour[kLane * 3], alpha[kLane];
    load_bytes<C>(rgb, base, n, cb);
#pragma unroll
    for (int j = 0; j < kLane; j++) {
#pragma unroll
        for (int k = 0; k < 3; k++) colour[3 * j + k] = unit(cb[C * j + k]);
        if (!kNormal) alpha[j] = unit(cb[C * j + C - 1]);
    }
    if (kNormal) {
        uint32_t nb[kLane * 4];
        float nrm[kLane * 3];
        load_bytes<4>(normal_rgba, base, n, nb);
#pragma unroll
        for (int j = 0; j < kLane; j++) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                float v = unit(nb[4 * j + k]) * 2.0f - 1.0f;
                if (k == 1) v = v * -1.0f;
                nrm[3 * j + k] = (v + 1.0f) / 2.0f;
            }
            alpha[j] = unit(nb[4 * j + 3]);
        }
        store_floats<3>(normal, base, n, nrm);
    }
    store_floats<1>(mask, base, n, alpha);
    store_floats<3>(rgb_out, base, n, colour);
}

bool aligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }
bool side_ok(int x) { return x >= 1 && x <= GD_VIEWS_MAX_SIDE; }

int refuse(const char* what, const char* why)
{
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: %s", what, why);
    return mesh_fail(-1, buf);
}

// -1 with a message, or 0
int validate_unpack(const char* what, int H, int W, int channels, bool present, bool all_aligned)
{
    if (!present) return refuse(what, "null pointer");
    if (!side_ok(H) || !side_ok(W)) return refuse(what, "H and W must be in [1, 8192]");
    if (channels != 3 && channels != 4) return refuse(what, "the colour image must have 3 or 4 channels");
    if (!all_aligned) return refuse(what, "every image must be 16-byte aligned");
    return 0;
}

dim3 unpack_grid(size_t npix) { return dim3((unsigned)((npix + kBlockPixels - 1) / kBlockPixels)); }

}  // namespace
}  // namespace gd

extern "C" {

int gd_views_png_unfilter(void* stream, const uint8_t* filtered, uint8_t* out, int B, int H, int W, int bpp)
{
    using namespace gd;
    const char* what = "views png_unfilter";
    if (!filtered || !out) return refuse(what, "null pointer");
    if (!side_ok(B) || !side_ok(H) || !side_ok(W)) return refuse(what, "B, H and W must be in [1, 8192]");
    if (bpp != 3 && bpp != 4) return refuse(what, "bpp must be 3 or 4");
    if (!aligned(filtered, 4) || !aligned(out, 4)) return refuse(what, "filtered and out must be 4-byte aligned");
    const size_t all = (size_t)B * H * ((size_t)W * bpp + 1);
    const int nchunks = (W + kChunk - 1) / kChunk;
    const int with_carry = H > kBand;
    const size_t lds = (size_t)kBand * kRing * bpp + (with_carry ? (size_t)nchunks * kChunk * bpp : 0);   // <= 64 KiB
    hipStream_t s = (hipStream_t)stream;
    if (bpp == 4)
        hipLaunchKernelGGL(png_unfilter_kernel<4>, dim3((unsigned)B), dim3(kBand), lds, s, filtered, out, all, H, W, with_carry);
    else
        hipLaunchKernelGGL(png_unfilter_kernel<3>, dim3((unsigned)B), dim3(kBand), lds, s, filtered, out, all, H, W, with_carry);
    return mesh_launched(nullptr, "views png_unfilter");
}

int gd_views_unpack(void* stream, const uint8_t* normal_rgba, const uint8_t* rgb, int rgb_channels, float* normal,
                    float* mask, float* rgb_out, int H, int W)
{
    using namespace gd;
    const bool present = normal_rgba && rgb && normal && mask && rgb_out;
    const bool all_aligned = aligned(normal_rgba, 16) && aligned(rgb, 16) && aligned(normal, 16) && aligned(mask, 16)
        && aligned(rgb_out, 16);
    if (validate_unpack("views unpack", H, W, rgb_channels, present, all_aligned)) return -1;
    const size_t npix = (size_t)H * W;
    hipStream_t s = (hipStream_t)stream;
    if (rgb_channels == 4)
        hipLaunchKernelGGL((unpack_kernel<4, true>), unpack_grid(npix), dim3(kBlock), 0, s, npix, normal_rgba, rgb, normal, mask,
                           rgb_out);
    else
        hipLaunchKernelGGL((unpack_kernel<3, true>), unpack_grid(npix), dim3(kBlock), 0, s, npix, normal_rgba, rgb, normal, mask,
                           rgb_out);
    return mesh_launched(nullptr, "views unpack");
}

int gd_views_unpack_rgba(void* stream, const uint8_t* rgba, float* rgb_out, float* mask, int H, int W)
{
    using namespace gd;
    const bool present = rgba && rgb_out && mask;
    const bool all_aligned = aligned(rgba, 16) && aligned(rgb_out, 16) && aligned(mask, 16);
    if (validate_unpack("views unpack_rgba", H, W, 4, present, all_aligned)) return -1;
    const size_t npix = (size_t)H * W;
    hipLaunchKernelGGL((unpack_kernel<4, false>), unpack_grid(npix), dim3(kBlock), 0, (hipStream_t)stream, npix,
                       (const uint8_t*)nullptr, rgba, (float*)nullptr, mask, rgb_out);
    return mesh_launched(nullptr, "views unpack_rgba");
}

}  // extern "C"
