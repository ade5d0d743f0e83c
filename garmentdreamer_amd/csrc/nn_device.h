// nn_device.h -- device primitives shared by every translation unit of libgd_nn.so (nn_*.hip and the nn_conv_*.h they
// include): bf16 conversion and packing, the vector types of the MFMA / packed-fp32 code, the LDS-DMA buffer load with
// its out-of-range sentinel, and the swizzle of the [rows][64] bf16 LDS tile.  One definition each, so that a fused
// epilogue rounds exactly like the separate kernel it replaces, and a tile written by one file is read back with the
// same swizzle and the same sentinel by another.  Everything here is __forceinline__: moving a helper into this header
// does not change the instructions of a kernel that uses it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gdnn {

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;     // MFMA bf16 operand fragment (8 x bf16 in 4 VGPRs)
typedef __attribute__((ext_vector_type(16))) float f32x16;      // 32x32 MFMA accumulator
typedef __attribute__((ext_vector_type(2))) float f32x2_t;      // operands of the packed fp32 VALU (v_pk_*_f32)
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
using f2 = f32x2_t;                                             // (short names of the packed row passes)
using bf2_t = bf16x2_t;

// 16 bytes = 8 x bf16 of HBM traffic: as eight halves, or as four words of two packed values (unpack2 / lo16 / hi16)
struct alignas(16) bf16x8 {
    uint16_t v[8];
};
struct alignas(16) u32x4 { uint32_t w[4]; };

__device__ __forceinline__ float bf2f(uint16_t b) { return __uint_as_float(((uint32_t)b) << 16); }
// fp32 -> bf16, round to nearest even, NaN kept quiet (scalar form; pack2 / pack_bf16 are the one-instruction pair form)
__device__ __forceinline__ uint16_t f2bf(float f)
{
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN
    u += 0x7fffu + ((u >> 16) & 1u);                                              // round to nearest even
    return (uint16_t)(u >> 16);
}

// Packed pairs: a 32-bit word holds two bf16, the even element in the low half.
__device__ __forceinline__ float lo16(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float hi16(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ f2 unpack2(uint32_t w) { return f2{lo16(w), hi16(w)}; }
// two fp32 -> packed bf16 (round to nearest even) in ONE instruction: v_cvt_pk_bf16_f32 (gfx950); the same bits as f2bf
// for every non-NaN input
__device__ __forceinline__ uint32_t pack2(f2 v) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf2_t)); }
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) { return pack2(f2{lo, hi}); }
__device__ __forceinline__ f2 round_bf16(f2 v) { return unpack2(pack2(v)); }

// ---- buffer addressing and LDS-DMA ----------------------------------------------------------------------------------
// Raw buffer descriptor over `bytes` bytes at p: stride 0, and the gfx9 flag word (DATA_FORMAT = 32) that the raw
// buffer instructions expect.  A lane whose voffset + instruction offset reaches `bytes` (num_records) is out of range:
// its load returns ZEROS and its store is dropped -- that is the halo padding and the ragged-tile masking of the
// kernels here, with no branch and no zero page.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, (int)bytes, 0x00020000);
}

constexpr uint32_t kOOB = 0x80000000u;   // voffset that fails the buffer range check (every tensor here is < 2 GiB)

// buffer_load_dwordx4 ... offen lds: 16 B per lane straight into LDS (wave-uniform base + lane * 16, no VGPR staging);
// out-of-range lanes (kOOB) write zeros.
__device__ __forceinline__ void bload_lds16(__amdgpu_buffer_rsrc_t rsrc, uint32_t voff, uint32_t soff, char* lds_wave_base)
{
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_wave_base, 16, voff, soff,
                                             0, 0);
}

// Byte offset of logical (row, 16-B chunk j) inside a swizzled tile image of 128-byte rows ([rows][64] bf16, or
// [rows][128] e4m3).  The image is 256-byte lines = two consecutive tile rows = 16 slots of 16 B; logical slot
// c = (row & 1) * 8 + j is stored at slot c ^ (line & 15): a 64-lane ds_read_b128 fragment read then touches 16
// distinct slots per 16-lane service group (conflict free).  LDS-DMA writes the image lane-linearly, so a loader
// applies the same permutation to WHICH (row, chunk) a lane fetches.
__device__ __forceinline__ int swz(int row, int j)
{
    return (row >> 1) * 256 + (((((row & 1) << 3) | j) ^ ((row >> 1) & 15)) << 4);
}

// ---- GroupNorm scale / shift table of the convolutions' activation loaders ------------------------------------------
// A loader that applies GroupNorm on the way to LDS computes x * sc + sh with sc = gamma[c] * rstd[n, g(c)] and
// sh = beta[c] - mean[n, g(c)] * sc.  Both depend on (image, channel) only, so a workgroup computes them ONCE per image into
// an LDS table and its K loop reads them back: no global load, no division by the group size and no bf16 conversion per
// chunk visit.  Layout: per channel octet o = c >> 3 sixteen floats {sc[0..7], sh[0..7]} = 64 contiguous bytes (the
// loaders own one octet of every pixel they move), 8 * Cin bytes in all.
constexpr int gn_table_bytes(int Cin) { return 8 * Cin; }

// One channel.  sh is ONE fused multiply-add (what hipcc's contraction made of `bt - mean * sc` before the table existed:
// the outputs keep their bits).
__device__ __forceinline__ void gn_scale_shift(float gm, float bt, float mean, float rstd, float& sc, float& sh)
{
    sc = gm * rstd;
    sh = __builtin_fmaf(-mean, sc, bt);
}

// Threads tid, tid + nthreads, ... each fill one channel of image `nimg` (one division per channel).  The caller puts
// gn_table_sync() between the fill and the first gn_table_read, and between the last read of an image and a refill.
// The LDS accesses of the table are inline asm: the compiler cannot tell a plain LDS access from the target of an LDS-DMA
// in flight and would put s_waitcnt vmcnt(0) in front of it.
__device__ __forceinline__ void gn_table_fill(uint32_t tab_off, int tid, int nthreads, int Cin, int G, int nimg,
                                              const float* __restrict__ mean_rstd, const uint16_t* __restrict__ gamma,
                                              const uint16_t* __restrict__ beta)
{
    const int cg = Cin / G;
    for (int ch = tid; ch < Cin; ch += nthreads) {
        const float2 mr = *(const float2*)(mean_rstd + ((size_t)nimg * G + ch / cg) * 2);
        float sc, sh;
        gn_scale_shift(bf2f(gamma[ch]), bf2f(beta[ch]), mr.x, mr.y, sc, sh);
        const uint32_t a = tab_off + (uint32_t)(((ch >> 3) * 16 + (ch & 7)) * 4);
        asm volatile("ds_write_b32 %0, %1\n\tds_write_b32 %0, %2 offset:32" ::"v"(a), "v"(sc), "v"(sh) : "memory");
    }
}

// The table's own barrier: waits for this wave's LDS operations only, not for global loads or LDS-DMA in flight.
__device__ __forceinline__ void gn_table_sync()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

// The sixteen values of one octet: four ds_read_b128 and their wait in ONE statement (the compiler does not count the
// loads of an asm statement: outputs are early-clobber and complete when the statement ends).
__device__ __forceinline__ void gn_table_read(uint32_t tab_off, int octet, float (&sc)[8], float (&sh)[8])
{
    typedef __attribute__((ext_vector_type(4))) float f32x4;
    f32x4 a, b, c, d;
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:16\n\tds_read_b128 %2, %4 offset:32\n\t"
                 "ds_read_b128 %3, %4 offset:48\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d)
                 : "v"(tab_off + (uint32_t)octet * 64u)
                 : "memory");
#pragma unroll
    for (int k = 0; k < 4; k++) { sc[k] = a[k]; sc[4 + k] = b[k]; sh[k] = c[k]; sh[4 + k] = d[k]; }
}

}  // namespace gdnn
