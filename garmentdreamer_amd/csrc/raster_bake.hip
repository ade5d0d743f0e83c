// raster_bake.hip -- the padding of the texture bake (C-ABI and the DEFINITIONS: include/gd_bake.h): for every texel of
// a UV atlas the nearest covered texel within the padding distance, and the gather that writes the 8-bit texture.
// Integers only; no atomics; every output element written.
//
//   pad index    one workgroup of 256 threads per 16 x 16 texel tile (a grid-stride loop over the tiles).  The coverage
//                of the tile and a halo of p texels goes to LDS ONCE, packed to one bit per texel: a wave reads 64
//                consecutive bytes of a mask row and __ballot is the word (16 + 2p <= 144 bits: three 64-bit words per
//                row, 3.4 KB at p = 64).  A tile whose haloed window is empty writes -1 and leaves; a covered texel
//                writes its own index and leaves.  Any other texel walks the rows r - p .. r + p in ascending order; in
//                a row the nearest set bit is the highest bit of the p columns to the left or the lowest of the p to
//                the right (clz / ctz of two 64-bit fields, left on equal distance: the lower index), so a row costs
//                two field extractions whatever p is.  A strict < across rows gives the header's tie rule.  Once a
//                witness of the L1 test is known, rows that cannot be strictly nearer are skipped.
//   resolve      one thread per texel.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_bake.h"

namespace gd {
namespace {

thread_local char g_bake_err[256] = "";

int bfail(int code, const char* what, const char* msg)
{
    snprintf(g_bake_err, sizeof(g_bake_err), "%s: %s", what, msg);
    return code;
}

constexpr int kTile = 16;
constexpr int kThreads = kTile * kTile;
constexpr int kWaves = kThreads / 64;
constexpr int kRowWords = 3;                                     // 64-bit words per staged row
constexpr int kMaxRows = kTile + 2 * GD_BAKE_MAX_PADDING;        // 144 rows and as many columns
constexpr int kMaxBlocks = 1 << 20;
static_assert(kMaxRows <= 64 * kRowWords, "a staged row must fit its words");

// 64 bits of a staged row from bit `pos` on (pos + 63 may reach into the next word, never past the row's last)
__device__ __forceinline__ unsigned long long field64(const unsigned long long* row, int pos)
{
    const int w = pos >> 6, s = pos & 63;
    unsigned long long v = row[w] >> s;
    if (s) v |= row[w + 1] << (64 - s);
    return v;
}

__global__ __launch_bounds__(kThreads) void pad_index_kernel(int H, int W, int p, int tiles_x, int64_t tiles,
                                                             const uint8_t* __restrict__ mask, int32_t* __restrict__ src)
{
    __shared__ unsigned long long s_bits[kMaxRows * kRowWords];
    __shared__ unsigned long long s_seen[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx = tid & (kTile - 1), ty = tid / kTile;
    const int span = kTile + 2 * p;                              // rows, and columns, of the haloed tile
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int r0 = (int)(tile / tiles_x) * kTile, c0 = (int)(tile % tiles_x) * kTile;
        unsigned long long seen = 0;
        for (int wi = wave; wi < span * kRowWords; wi += kWaves) {           // wave-uniform: all 64 lanes vote
            const int row = wi / kRowWords, first = (wi - row * kRowWords) * 64;
            unsigned long long word = 0;
            if (first < span) {
                const int col = first + lane, r = r0 - p + row, c = c0 - p + col;
                bool covered = false;
                if (col < span && r >= 0 && r < H && c >= 0 && c < W) covered = mask[(int64_t)r * W + c] != 0;
                word = __ballot(covered);
            }
            seen |= word;
            if (lane == 0) s_bits[wi] = word;
        }
        if (lane == 0) s_seen[wave] = seen;
        __syncthreads();
        const int r = r0 + ty, c = c0 + tx;
        if (r < H && c < W) {
            const int x = tx + p;                                            // own column in the staged rows
            const unsigned long long* own = s_bits + (ty + p) * kRowWords;
            int32_t out = -1;
            if ((own[x >> 6] >> (x & 63)) & 1) {
                out = r * W + c;
            } else if (p > 0 && (s_seen[0] | s_seen[1] | s_seen[2] | s_seen[3]) != 0) {
                const unsigned long long keep = p == 64 ? ~0ull : (1ull << p) - 1;
                int best = INT_MAX, best_dr = 0, best_dc = 0;
                bool witness = false;                                        // some covered texel within L1 distance p
                for (int dr = -p; dr <= p; dr++) {
                    if (witness && dr * dr >= best) {                        // only a strictly nearer texel could win
                        if (dr > 0) break;
                        continue;
                    }
                    const unsigned long long* row = s_bits + (ty + p + dr) * kRowWords;
                    int dc;
                    if ((row[x >> 6] >> (x & 63)) & 1) {
                        dc = 0;
                    } else {
                        const unsigned long long left = field64(row, tx) & keep;       // bit i: column x - p + i
                        const unsigned long long right = field64(row, x + 1) & keep;   // bit i: column x + 1 + i
                        if (!(left | right)) continue;
                        const int dl = left ? p - 63 + __builtin_clzll(left) : INT_MAX;
                        const int dq = right ? __builtin_ctzll(right) + 1 : INT_MAX;
                        dc = dl <= dq ? -dl : dq;
                    }
                    const int adr = dr < 0 ? -dr : dr, adc = dc < 0 ? -dc : dc;
                    witness |= adr + adc <= p;
                    const int d2 = dr * dr + dc * dc;
                    if (d2 < best) {
                        best = d2;
                        best_dr = dr;
                        best_dc = dc;
                    }
                }
                if (witness) out = (r + best_dr) * W + (c + best_dc);
            }
            src[(int64_t)r * W + c] = out;
        }
        __syncthreads();                                                     // the next tile restages s_bits
    }
}

__global__ __launch_bounds__(256) void resolve_u8_kernel(int64_t n, int C, const float* __restrict__ image,
                                                         const int32_t* __restrict__ src, uint8_t* __restrict__ out)
{
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
        const int32_t s = src[t];
        const bool follow = s >= 0 && s < n;
        for (int k = 0; k < C; k++) {
            uint8_t q = 0;
            if (follow) {
                float x = image[(int64_t)s * C + k];
                x = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;                 // NaN compares false: 0
                q = (uint8_t)(int)(x * 255.0f);
            }
            out[t * C + k] = q;
        }
    }
}

int check_image(const char* what, int H, int W)
{
    if (H < 1 || W < 1) return bfail(-1, what, "H and W must be at least 1");
    if ((int64_t)H * W >= ((int64_t)1 << 31)) return bfail(-1, what, "H W must be below 2^31");
    return 0;
}

int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : bfail(-2, what, hipGetErrorString(e));
}

}  // namespace
}  // namespace gd

extern "C" {

int gd_bake_pad_index(void* stream, int H, int W, int padding, const uint8_t* mask, int32_t* src)
{
    using namespace gd;
    const char* what = "pad index";
    if (!mask || !src) return bfail(-1, what, "null pointer");
    if (int r = check_image(what, H, W)) return r;
    if (padding < 0 || padding > GD_BAKE_MAX_PADDING) return bfail(-1, what, "padding must be in 0..64");
    const int tiles_x = (W + kTile - 1) / kTile;
    const int64_t tiles = (int64_t)tiles_x * ((H + kTile - 1) / kTile);
    const unsigned blocks = (unsigned)(tiles < kMaxBlocks ? tiles : kMaxBlocks);
    hipLaunchKernelGGL(pad_index_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, H, W, padding, tiles_x,
                       tiles, mask, src);
    return launched(what);
}

int gd_bake_resolve_u8(void* stream, int H, int W, int C, const float* image, const int32_t* src, uint8_t* out)
{
    using namespace gd;
    const char* what = "resolve u8";
    if (!image || !src || !out) return bfail(-1, what, "null pointer");
    if (int r = check_image(what, H, W)) return r;
    if (C < 1 || C > GD_BAKE_MAX_CHANNELS) return bfail(-1, what, "C must be in 1..4");
    const int64_t n = (int64_t)H * W;
    const int64_t want = (n + 255) / 256;
    const unsigned blocks = (unsigned)(want < kMaxBlocks ? want : kMaxBlocks);
    hipLaunchKernelGGL(resolve_u8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, C, image, src, out);
    return launched(what);
}

const char* gd_bake_last_error(void) { return gd::g_bake_err; }

}  // extern "C"
