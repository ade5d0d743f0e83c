// raster_texture_sorted.hip -- the texture field's bit-reproducible grid gradient (DEFINITION and C-ABI:
// include/gd_texture_sorted.h; the entries are in raster_texture.hip): the contributions of a level are sorted by
// destination with a stable radix sort and every destination adds its own run in order.  Built with -ffp-contract=off.
//
// Levels go in groups of kSortedGroup, the level of a workgroup on blockIdx.y (slot = blockIdx.y of the scratch arrays).
// M = 8 N items per level, item id 8 n + i.
//   sorted_keys      one thread per point: the 8 keys idx_i at positions 8 n .. 8 n + 7 (two 16-byte stores); size_l for a
//                    point that takes no part: one more than the largest index, so it sorts last
//   sorted_hist / sorted_scan / sorted_scatter
//                    one pass of the LSD sort over an 8-bit digit, after raster_binning.hip's radix_* (a copy for 32-bit
//                    keys: those kernels have their own bit-identity tests and are not touched): digit counts per
//                    2 048-item tile, an exclusive scan per digit over the tiles, and a scatter that ranks every key inside
//                    its wave by ballot, in (wave, step, lane) order, which is ascending position: stable.  A level needs
//                    ceil(bit_length(size_l) / 8) passes (the sentinel size_l included); a workgroup of a level that is
//                    done returns, and the level's result sits in buffer (passes & 1).  Pass 0 takes the item id from the
//                    position instead of reading it.
//   sorted_contrib   one thread per sorted position: weight_i * denc of its item, a float2, in sorted order
//   sorted_sum       one thread per sorted position; the first position of an entry adds the entry's contiguous run from
//                    +0 in order (8 positions loaded ahead per step: the loads of a step do not wait for each other) and
//                    adds the sum to dgrid with a plain load and store.  Entries are distinct across threads: no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "raster_texture_cells.h"

namespace gd {
namespace {

constexpr int kSortedGroup = 4;                               // levels per group of launches
constexpr int kSortedItems = 8;                               // keys per thread of a sort workgroup
constexpr uint32_t kSortedTile = 256 * kSortedItems;          // 2 048 keys per sort workgroup
constexpr int kSortedBits = 8, kSortedBins = 1 << kSortedBits;
constexpr int kSumAhead = 8;

struct SortedScratch {
    uint32_t* keys[2];      // [group][Mp] each
    uint32_t* vals[2];
    float2* contrib;        // [group][Mp]
    uint32_t* hist;         // [group][kSortedBins][nblk]
    uint32_t* totals;       // [group][kSortedBins]
    size_t Mp;              // M rounded up to 64 items: every array starts 256-byte aligned
    uint32_t M, nblk;
};

__host__ __device__ __forceinline__ int sorted_passes(uint32_t size)
{
    int bits = 0;
    while (bits < 32 && (size >> bits) != 0) bits++;          // bit_length(size): the keys are 0 .. size, size > 0
    return (bits + kSortedBits - 1) / kSortedBits;
}

__global__ __launch_bounds__(256) void sorted_keys_kernel(int N, int first, const float* __restrict__ x,
                                                          const uint8_t* __restrict__ mask, gd_texture_layout lay,
                                                          SortedScratch sc)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const Level lv = level_of(lay, first + (int)blockIdx.y);
    float u[3];
    uint32_t k[8];
    if (load_point(n, N, x, mask, u)) {
        const Cell ce = cell_of(u, lv.scale);
#pragma unroll
        for (int i = 0; i < 8; i++) k[i] = corner_index(lv, ce, i);
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++) k[i] = lv.size;
    }
    uint4* dst = reinterpret_cast<uint4*>(sc.keys[0] + blockIdx.y * sc.Mp + 8 * (size_t)n);   // 8 n + 7 < M <= Mp
    dst[0] = make_uint4(k[0], k[1], k[2], k[3]);
    dst[1] = make_uint4(k[4], k[5], k[6], k[7]);
}

__global__ __launch_bounds__(256) void sorted_hist_kernel(int first, int pass, gd_texture_layout lay, SortedScratch sc)
{
    if (pass >= sorted_passes((uint32_t)lay.size[first + blockIdx.y])) return;
    const uint32_t* keys = sc.keys[pass & 1] + blockIdx.y * sc.Mp;
    uint32_t* hist = sc.hist + (size_t)blockIdx.y * kSortedBins * sc.nblk;
    const int shift = pass * kSortedBits;
    __shared__ uint32_t h[kSortedBins];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * kSortedTile;
#pragma unroll
    for (int k = 0; k < kSortedItems; k++) {
        const uint32_t idx = base + k * 256 + threadIdx.x;
        if (idx < sc.M) atomicAdd(&h[(keys[idx] >> shift) & (kSortedBins - 1)], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * sc.nblk + blockIdx.x] = h[threadIdx.x];
}

// one workgroup per (digit, level): exclusive scan of hist[d][0 .. nblk) in place, the digit's total to totals[d]
__global__ __launch_bounds__(256) void sorted_scan_kernel(int first, int pass, gd_texture_layout lay, SortedScratch sc)
{
    if (pass >= sorted_passes((uint32_t)lay.size[first + blockIdx.y])) return;
    __shared__ uint32_t wave_incl[4];
    __shared__ uint32_t carry_s;
    const uint32_t nblk = sc.nblk;
    uint32_t* row = sc.hist + ((size_t)blockIdx.y * kSortedBins + blockIdx.x) * nblk;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nblk; base += 256) {
        const uint32_t i = base + tid;
        const uint32_t v = i < nblk ? row[i] : 0;
        uint32_t incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            uint32_t t = __shfl_up(incl, off, 64);
            if (lane >= (uint32_t)off) incl += t;
        }
        if (lane == 63) wave_incl[wave] = incl;
        __syncthreads();
        uint32_t wave_off = 0;
        for (uint32_t w = 0; w < wave; w++) wave_off += wave_incl[w];
        const uint32_t carry = carry_s;
        if (i < nblk) row[i] = carry + wave_off + incl - v;
        __syncthreads();
        if (tid == 255) carry_s = carry + wave_off + incl;
        __syncthreads();
    }
    if (tid == 0) sc.totals[blockIdx.y * kSortedBins + blockIdx.x] = carry_s;
}

__global__ __launch_bounds__(256) void sorted_scatter_kernel(int first, int pass, gd_texture_layout lay, SortedScratch sc)
{
    if (pass >= sorted_passes((uint32_t)lay.size[first + blockIdx.y])) return;
    const size_t slot = blockIdx.y * sc.Mp;
    const uint32_t* keys_in = sc.keys[pass & 1] + slot;
    const uint32_t* vals_in = sc.vals[pass & 1] + slot;
    uint32_t* keys_out = sc.keys[(pass + 1) & 1] + slot;
    uint32_t* vals_out = sc.vals[(pass + 1) & 1] + slot;
    const uint32_t* hist = sc.hist + (size_t)blockIdx.y * kSortedBins * sc.nblk;
    const uint32_t* totals = sc.totals + blockIdx.y * kSortedBins;
    const uint32_t n = sc.M, nblk = sc.nblk;
    const int shift = pass * kSortedBits;

    __shared__ uint32_t cnt[4][kSortedBins];    // per-wave running digit counts, later wave bases
    __shared__ uint32_t dbase[kSortedBins];     // global base of digit d for this workgroup
    __shared__ uint32_t wave_tot[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // exclusive scan of the digit totals (one per thread) + this workgroup's offset inside each digit
    const uint32_t mine = totals[tid];
    uint32_t incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        uint32_t t = __shfl_up(incl, off, 64);
        if (lane >= (uint32_t)off) incl += t;
    }
    if (lane == 63) wave_tot[wave] = incl;
    for (int i = tid; i < 4 * kSortedBins; i += 256) (&cnt[0][0])[i] = 0;
    __syncthreads();
    uint32_t run = incl - mine;
    for (uint32_t w = 0; w < wave; w++) run += wave_tot[w];
    dbase[tid] = run + hist[(size_t)tid * nblk + blockIdx.x];
    __syncthreads();

    // rank every key inside its wave: element idx of the tile belongs to wave idx / 512, inside it (step, lane)
    const uint32_t base = blockIdx.x * kSortedTile + wave * (64 * kSortedItems);
    uint32_t key[kSortedItems];
    uint32_t rank[kSortedItems];
    volatile uint32_t* wc = cnt[wave];
    const uint64_t lt_mask = (1ull << lane) - 1ull;
#pragma unroll
    for (int s = 0; s < kSortedItems; s++) {
        const uint32_t idx = base + s * 64 + lane;
        const bool valid = idx < n;
        key[s] = valid ? keys_in[idx] : ~0u;
        const uint32_t d = (key[s] >> shift) & (kSortedBins - 1);
        uint64_t peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < kSortedBits; b++) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t before = (uint32_t)__popcll(peers & lt_mask);
        uint32_t r = 0;
        if (valid) {
            const uint32_t c = wc[d];
            r = c + before;
            if (before == 0) wc[d] = c + (uint32_t)__popcll(peers);
        }
        rank[s] = r;
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // per-wave counts into per-wave bases (exclusive over the waves) + the global digit base
    {
        uint32_t run2 = dbase[tid];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t c = cnt[w][tid];
            cnt[w][tid] = run2;
            run2 += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kSortedItems; s++) {
        const uint32_t idx = base + s * 64 + lane;
        if (idx < n) {
            const uint32_t d = (key[s] >> shift) & (kSortedBins - 1);
            const uint32_t pos = cnt[wave][d] + rank[s];      // < n: the ranks of all n keys are a permutation of 0 .. n-1
            keys_out[pos] = key[s];
            vals_out[pos] = pass == 0 ? idx : vals_in[idx];
        }
    }
}

__global__ __launch_bounds__(256) void sorted_contrib_kernel(int N, int first, const float* __restrict__ x,
                                                             const uint8_t* __restrict__ mask,
                                                             const float* __restrict__ denc, gd_texture_layout lay,
                                                             SortedScratch sc)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= sc.M) return;
    const int l = first + (int)blockIdx.y;
    const Level lv = level_of(lay, l);
    const int buf = sorted_passes(lv.size) & 1;
    const size_t slot = blockIdx.y * sc.Mp;
    if (sc.keys[buf][slot + j] == lv.size) return;            // a point that takes no part: never summed
    const uint32_t item = sc.vals[buf][slot + j];             // 8 n + i, n < N
    const int n = (int)(item >> 3), i = (int)(item & 7);
    float u[3];
    if (!load_point(n, N, x, mask, u)) return;                // (it takes part: it has a key)
    const Cell ce = cell_of(u, lv.scale);
    const float w = corner_weight(ce, i);
    const float* d = denc + (size_t)n * lay.num_levels * GD_TEXTURE_FEATURES + 2 * l;
    sc.contrib[slot + j] = make_float2(w * d[0], w * d[1]);
}

__global__ __launch_bounds__(256) void sorted_sum_kernel(int first, gd_texture_layout lay, SortedScratch sc,
                                                         float* __restrict__ dgrid)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    const uint32_t M = sc.M;
    if (j >= M) return;
    const Level lv = level_of(lay, first + (int)blockIdx.y);
    const uint32_t* keys = sc.keys[sorted_passes(lv.size) & 1] + blockIdx.y * sc.Mp;
    const float2* contrib = sc.contrib + blockIdx.y * sc.Mp;
    const uint32_t k = keys[j];
    if (k == lv.size) return;
    if (j > 0 && keys[j - 1] == k) return;                    // not the first position of its entry
    float s0 = 0.0f, s1 = 0.0f;
    bool more = true;
    for (uint32_t t = j; more; t += kSumAhead) {
        uint32_t kk[kSumAhead];
        float2 cc[kSumAhead];
#pragma unroll
        for (int a = 0; a < kSumAhead; a++) {
            const uint32_t idx = t + a < M ? t + a : M - 1;   // clamped: what lies beyond the run is loaded, never added
            kk[a] = keys[idx];
            cc[a] = contrib[idx];
        }
#pragma unroll
        for (int a = 0; a < kSumAhead; a++) {
            more = more && t + a < M && kk[a] == k;
            if (more) {
                s0 = s0 + cc[a].x;
                s1 = s1 + cc[a].y;
            }
        }
    }
    float* dst = dgrid + ((size_t)lv.offset + k) * GD_TEXTURE_FEATURES;   // k < size_l: inside the level
    dst[0] = dst[0] + s0;
    dst[1] = dst[1] + s1;
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int group_levels(const gd_texture_layout& lay) { return lay.num_levels < kSortedGroup ? lay.num_levels : kSortedGroup; }

// the arrays of the scratch, one after the other; returns the bytes
size_t carve(int N, const gd_texture_layout& lay, void* scratch, SortedScratch* sc)
{
    const size_t G = (size_t)group_levels(lay);
    const size_t M = 8 * (size_t)N;
    const size_t Mp = (M + 63) & ~(size_t)63;
    const size_t nblk = (M + kSortedTile - 1) / kSortedTile;
    char* p = (char*)scratch;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char* r = p + off;
        off += align256(bytes);
        return r;
    };
    SortedScratch s;
    s.keys[0] = (uint32_t*)take(G * Mp * 4);
    s.keys[1] = (uint32_t*)take(G * Mp * 4);
    s.vals[0] = (uint32_t*)take(G * Mp * 4);
    s.vals[1] = (uint32_t*)take(G * Mp * 4);
    s.contrib = (float2*)take(G * Mp * 8);
    s.hist = (uint32_t*)take(G * kSortedBins * nblk * 4);
    s.totals = (uint32_t*)take(G * kSortedBins * 4);
    s.Mp = Mp;
    s.M = (uint32_t)M;
    s.nblk = (uint32_t)nblk;
    if (sc) *sc = s;
    return off;
}

}  // namespace

size_t sorted_dgrid_scratch_bytes(int N, const gd_texture_layout& lay) { return carve(N, lay, nullptr, nullptr); }

void launch_sorted_dgrid(hipStream_t s, int N, const float* x, const uint8_t* mask, const float* denc,
                         const gd_texture_layout& lay, float* dgrid, void* scratch)
{
    SortedScratch sc;
    carve(N, lay, scratch, &sc);
    const unsigned per_point = (unsigned)(((int64_t)N + 255) / 256), per_item = (unsigned)((sc.M + 255) / 256);
    for (int first = 0; first < lay.num_levels; first += kSortedGroup) {
        const unsigned nlev = (unsigned)(lay.num_levels - first < kSortedGroup ? lay.num_levels - first : kSortedGroup);
        int passes = 0;
        for (unsigned g = 0; g < nlev; g++) {
            const int p = sorted_passes((uint32_t)lay.size[first + g]);
            passes = p > passes ? p : passes;
        }
        hipLaunchKernelGGL(sorted_keys_kernel, dim3(per_point, nlev), dim3(256), 0, s, N, first, x, mask, lay, sc);
        for (int pass = 0; pass < passes; pass++) {
            hipLaunchKernelGGL(sorted_hist_kernel, dim3(sc.nblk, nlev), dim3(256), 0, s, first, pass, lay, sc);
            hipLaunchKernelGGL(sorted_scan_kernel, dim3(kSortedBins, nlev), dim3(256), 0, s, first, pass, lay, sc);
            hipLaunchKernelGGL(sorted_scatter_kernel, dim3(sc.nblk, nlev), dim3(256), 0, s, first, pass, lay, sc);
        }
        hipLaunchKernelGGL(sorted_contrib_kernel, dim3(per_item, nlev), dim3(256), 0, s, N, first, x, mask, denc, lay, sc);
        hipLaunchKernelGGL(sorted_sum_kernel, dim3(per_item, nlev), dim3(256), 0, s, first, lay, sc, dgrid);
    }
}

}  // namespace gd
