// nn_vae_decoder.hip -- the two ends of the SD-2.1 VAE decoder (diffusers AutoencoderKL.decode) that no other kernel of
// the package covers; everything between them (ResnetBlock2D, the d = 512 mid attention, Upsample2D) runs on the
// encoder's / UNet's kernels.
//
//   gd_nn_vae_decoder_stem
//       z = latents * inv_scale;  p = post_quant_conv(z)  (1x1, 4 -> 4);  y = conv_in(p)  (3x3, pad 1, 4 -> Cout)
//     One launch.  A workgroup owns an 8 x 8 pixel tile: it computes the post-quant values of the 10 x 10 halo into LDS
//     (zero outside the image -- the padding belongs to the post-quant tensor, so post_quant_conv is NOT folded into
//     conv_in's weights: the border pixels would differ) and keeps the whole 36 x Cout conv_in filter bank (36 KiB bf16
//     at Cout = 512) in LDS.  A thread computes 8 output channels of 4 pixels in fp32 and writes them as one 16-byte
//     vector per pixel: bf16 NHWC, the layout the first ResnetBlock2D reads.  36 MACs per output: a VALU kernel.
//
//   gd_nn_vae_decoder_head
//       y = conv_out(silu(GroupNorm(x)))  (3x3, pad 1, C -> 3)  [ -> clamp(y * 0.5 + 0.5, 0, 1) ]
//     One launch, one pass over x.  A workgroup owns a 16 x 16 pixel tile and walks the channels in slices of 64: the
//     18 x 18 halo slice is read with 16-byte loads (one 128-byte line per pixel and slice; the next slice's loads are in
//     flight while the current one is consumed), normalised with the
//     per-image statistics, passed through SiLU, rounded to bf16 (as the eager bf16 ops round the activation) and
//     staged in LDS; each thread then accumulates its pixel's three outputs with v_dot2_f32_bf16 against weights read
//     through the scalar cache (wave-uniform addresses).  No atomics: every output element is written exactly once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/gd_nn.h"
#include "nn_device.h"
#include "nn_host.h"
#include "nn_math.h"

namespace {

using namespace gdnn;

template <bool BF16_IN> __device__ __forceinline__ float load_in(const void* p, int64_t i)
{
    if constexpr (BF16_IN) return bf2f(((const uint16_t*)p)[i]);
    else return ((const float*)p)[i];
}

// ---- stem ---------------------------------------------------------------------------------------------------------
constexpr int ST_T = 8;               // output tile edge
constexpr int ST_H = ST_T + 2;        // halo tile edge
constexpr int ST_MAX_COUT = 512;

template <bool BF16_IN>
__global__ __launch_bounds__(256) void stem_kernel(const void* __restrict__ lat, float inv_scale,
                                                   const uint16_t* __restrict__ pq_w, const uint16_t* __restrict__ pq_b,
                                                   const uint16_t* __restrict__ w, const uint16_t* __restrict__ b,
                                                   uint16_t* __restrict__ y, int h, int wd, int Cout)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_w[36 * ST_MAX_COUT];   // [tap * 4 + ci][Cout]
    __shared__ __attribute__((aligned(16))) float s_p[ST_H * ST_H * 4];        // post-quant halo, [pixel][ci]
    __shared__ float s_pq[20];                                                 // 4 x 4 weights + 4 biases
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int ty0 = blockIdx.y * ST_T, tx0 = blockIdx.x * ST_T;

    if (tid < 16) s_pq[tid] = bf2f(pq_w[tid]);
    else if (tid < 20) s_pq[tid] = pq_b ? bf2f(pq_b[tid - 16]) : 0.f;
    // conv_in weights [Cout][3][3][4] (channels_last storage) -> [k = tap * 4 + ci][Cout]
    for (int i = tid; i < 36 * Cout; i += 256) {
        const int co = i / 36, k = i - co * 36;
        s_w[k * Cout + co] = w[i];
    }
    __syncthreads();
    const int64_t plane = (int64_t)h * wd;
    for (int i = tid; i < ST_H * ST_H; i += 256) {
        const int hy = i / ST_H, hx = i - hy * ST_H;
        const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (gy >= 0 && gy < h && gx >= 0 && gx < wd) {
            const int64_t base = (int64_t)n * 4 * plane + (int64_t)gy * wd + gx;
            float z[4];
#pragma unroll
            for (int c = 0; c < 4; c++) z[c] = load_in<BF16_IN>(lat, base + c * plane) * inv_scale;
#pragma unroll
            for (int co = 0; co < 4; co++)
                o[co] = s_pq[16 + co] + s_pq[co * 4 + 0] * z[0] + s_pq[co * 4 + 1] * z[1] + s_pq[co * 4 + 2] * z[2] +
                        s_pq[co * 4 + 3] * z[3];
        }
        *(float4*)&s_p[i * 4] = make_float4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();

    // work item = (pixel quad, channel group of 8): 16 quads (8 x 8 tile, 2 quads per row) x Cout / 8 groups
    const int groups = Cout >> 3;
    for (int item = tid; item < 16 * groups; item += 256) {
        const int cg = item % groups, quad = item / groups;
        const int r = quad >> 1, c0 = (quad & 1) * 4;
        float acc[4][8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float bj = b ? bf2f(b[cg * 8 + j]) : 0.f;
#pragma unroll
            for (int q = 0; q < 4; q++) acc[q][j] = bj;
        }
#pragma unroll 1
        for (int ky = 0; ky < 3; ky++) {
#pragma unroll
            for (int kx = 0; kx < 3; kx++) {
#pragma unroll
                for (int ci = 0; ci < 4; ci++) {
                    const uint4 wv = *(const uint4*)&s_w[((ky * 3 + kx) * 4 + ci) * Cout + cg * 8];
                    const f2 w01 = unpack2(wv.x), w23 = unpack2(wv.y), w45 = unpack2(wv.z), w67 = unpack2(wv.w);
                    const float wf[8] = {w01.x, w01.y, w23.x, w23.y, w45.x, w45.y, w67.x, w67.y};
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const float a = s_p[((r + ky) * ST_H + c0 + q + kx) * 4 + ci];
#pragma unroll
                        for (int j = 0; j < 8; j++) acc[q][j] = fmaf(wf[j], a, acc[q][j]);
                    }
                }
            }
        }
        const int gy = ty0 + r;
        if (gy >= h) continue;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int gx = tx0 + c0 + q;
            if (gx >= wd) continue;
            uint4 v;
            v.x = pack2(f2{acc[q][0], acc[q][1]});
            v.y = pack2(f2{acc[q][2], acc[q][3]});
            v.z = pack2(f2{acc[q][4], acc[q][5]});
            v.w = pack2(f2{acc[q][6], acc[q][7]});
            *(uint4*)&y[(((int64_t)n * h + gy) * wd + gx) * Cout + cg * 8] = v;
        }
    }
}

// ---- head ---------------------------------------------------------------------------------------------------------
constexpr int HD_T = 16;               // output tile edge: one pixel per thread
constexpr int HD_H = HD_T + 2;         // halo tile edge
constexpr int HD_SLICE = 64;           // channels staged per pass
constexpr int HD_PITCH = 36;           // dwords per staged pixel: 32 + 4 pad (16 lanes of a row read 16 distinct bank quads)
constexpr int HD_MAX_C = 256;

constexpr int HD_PIECES = (HD_H * HD_H * 8 + 255) / 256;   // 16-byte pieces of a halo slice per thread

// the raw pieces of one halo slice (channels c0 .. c0 + 63 of the 18 x 18 pixels), zeros outside the image
__device__ __forceinline__ void load_slice(const uint16_t* __restrict__ x, uint4 (&pre)[HD_PIECES], int c0, int n, int ty0,
                                           int tx0, int H, int W, int C, int tid)
{
#pragma unroll
    for (int j = 0; j < HD_PIECES; j++) {
        const int i = tid + j * 256;
        const int px = i >> 3, q = i & 7;
        const int hy = px / HD_H, hx = px - hy * HD_H;
        const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
        pre[j] = make_uint4(0u, 0u, 0u, 0u);
        if (i < HD_H * HD_H * 8 && gy >= 0 && gy < H && gx >= 0 && gx < W)
            pre[j] = *(const uint4*)&x[(((int64_t)n * H + gy) * W + gx) * C + c0 + q * 8];
    }
}

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) u32x4_t* const_u4_ptr;   // scalar-cache loads (uniform addresses)

template <int MODE>
__global__ __launch_bounds__(256) void head_kernel(const uint16_t* __restrict__ x, const float* __restrict__ mean_rstd,
                                                   const uint16_t* __restrict__ gamma, const uint16_t* __restrict__ beta,
                                                   int G, const uint16_t* __restrict__ w, const uint16_t* __restrict__ b,
                                                   void* __restrict__ out, int H, int W, int C)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_a[HD_H * HD_H * HD_PITCH];
    __shared__ float s_scale[HD_MAX_C], s_shift[HD_MAX_C];
    const int tid = threadIdx.x;
    const int n = blockIdx.z;
    const int ty0 = blockIdx.y * HD_T, tx0 = blockIdx.x * HD_T;
    // GroupNorm as one fma per channel: silu(x * scale + shift), scale = rstd * gamma, shift = beta - mean * scale
    const int cpg = C / G;
    for (int c = tid; c < C; c += 256) {
        const int g = c / cpg;
        const float mean = mean_rstd[((int64_t)n * G + g) * 2], rstd = mean_rstd[((int64_t)n * G + g) * 2 + 1];
        const float s = rstd * bf2f(gamma[c]);
        s_scale[c] = s;
        s_shift[c] = bf2f(beta[c]) - mean * s;
    }
    const_u4_ptr wc = (const_u4_ptr)w;       // [3][3][3][C] (channels_last storage of conv_out.weight), 8 channels per uint4
    const int ty = tid >> 4, tx = tid & 15;
    float acc0 = b ? bf2f(b[0]) : 0.f, acc1 = b ? bf2f(b[1]) : 0.f, acc2 = b ? bf2f(b[2]) : 0.f;

    // the halo slice is HD_PIECES 16-byte pieces per thread; the next slice's pieces are loaded into registers while the
    // current one is consumed, so the loads' latency hides behind the dot products
    uint4 pre[HD_PIECES];
    load_slice(x, pre, 0, n, ty0, tx0, H, W, C, tid);
    for (int c0 = 0; c0 < C; c0 += HD_SLICE) {
        __syncthreads();      // statistics visible (first slice) / previous slice consumed
#pragma unroll
        for (int j = 0; j < HD_PIECES; j++) {
            const int i = tid + j * 256;
            if (i >= HD_H * HD_H * 8) break;
            const int px = i >> 3, q = i & 7;
            const int hy = px / HD_H, hx = px - hy * HD_H;
            const int gy = ty0 - 1 + hy, gx = tx0 - 1 + hx;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);        // conv padding: zeros of silu(GroupNorm(x))
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const int c = c0 + q * 8;
                const uint32_t rw[4] = {pre[j].x, pre[j].y, pre[j].z, pre[j].w};
                uint32_t o[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const f2 s = {s_scale[c + 2 * k], s_scale[c + 2 * k + 1]};
                    const f2 t = {s_shift[c + 2 * k], s_shift[c + 2 * k + 1]};
                    const f2 u = unpack2(rw[k]) * s + t;
                    const f2 e = {__builtin_amdgcn_exp2f(u.x * -1.44269504088896341f),
                                  __builtin_amdgcn_exp2f(u.y * -1.44269504088896341f)};
                    const f2 d = 1.0f + e;
                    o[k] = pack2(u * f2{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)});
                }
                v = make_uint4(o[0], o[1], o[2], o[3]);
            }
            *(uint4*)&s_a[px * HD_PITCH + q * 4] = v;
        }
        __syncthreads();
        if (c0 + HD_SLICE < C) load_slice(x, pre, c0 + HD_SLICE, n, ty0, tx0, H, W, C, tid);
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int ky = tap / 3, kx = tap - ky * 3;
            const uint32_t* ap = &s_a[((ty + ky) * HD_H + tx + kx) * HD_PITCH];
#pragma unroll
            for (int k8 = 0; k8 < HD_SLICE / 8; k8++) {
                const uint4 a = *(const uint4*)&ap[k8 * 4];
                const int wi = (c0 + k8 * 8) >> 3;
                const u32x4_t w0 = wc[(0 * 9 + tap) * (C >> 3) + wi];
                const u32x4_t w1 = wc[(1 * 9 + tap) * (C >> 3) + wi];
                const u32x4_t w2 = wc[(2 * 9 + tap) * (C >> 3) + wi];
                const uint32_t av[4] = {a.x, a.y, a.z, a.w};
                const uint32_t v0[4] = {w0.x, w0.y, w0.z, w0.w}, v1[4] = {w1.x, w1.y, w1.z, w1.w},
                               v2[4] = {w2.x, w2.y, w2.z, w2.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const bf2_t ak = __builtin_bit_cast(bf2_t, av[k]);
                    acc0 = __builtin_amdgcn_fdot2_f32_bf16(ak, __builtin_bit_cast(bf2_t, v0[k]), acc0, false);
                    acc1 = __builtin_amdgcn_fdot2_f32_bf16(ak, __builtin_bit_cast(bf2_t, v1[k]), acc1, false);
                    acc2 = __builtin_amdgcn_fdot2_f32_bf16(ak, __builtin_bit_cast(bf2_t, v2[k]), acc2, false);
                }
            }
        }
    }
    const int gy = ty0 + ty, gx = tx0 + tx;
    if (gy >= H || gx >= W) return;
    const int64_t o = (((int64_t)n * H + gy) * W + gx) * 3;
    if constexpr (MODE == GD_NN_VAE_HEAD_RAW) {
        uint16_t* yo = (uint16_t*)out;
        yo[o] = f2bf(acc0);
        yo[o + 1] = f2bf(acc1);
        yo[o + 2] = f2bf(acc2);
    } else {
        float* yo = (float*)out;
        yo[o] = fminf(fmaxf(fmaf(acc0, 0.5f, 0.5f), 0.f), 1.f);
        yo[o + 1] = fminf(fmaxf(fmaf(acc1, 0.5f, 0.5f), 0.f), 1.f);
        yo[o + 2] = fminf(fmaxf(fmaf(acc2, 0.5f, 0.5f), 0.f), 1.f);
    }
}

constexpr int64_t I31 = (int64_t)1 << 31;

}  // namespace

extern "C" {

int gd_nn_vae_decoder_stem_supported(int N, int h, int w, int Cout)
{
    if (N < 1 || h < 1 || w < 1 || N > 65535) return 0;
    if (Cout < 64 || Cout > ST_MAX_COUT || Cout % 64) return 0;
    if ((int64_t)N * h * w * Cout >= I31) return 0;
    return 1;
}

int gd_nn_vae_decoder_stem(void* stream, const void* latents, int latents_bf16, float inv_scale, const void* pq_weight,
                           const void* pq_bias, const void* weight, const void* bias, void* y, int N, int h, int w, int Cout)
{
    if (!latents || !pq_weight || !weight || !y) return fail(GD_NN_ERR_INVALID_ARG, "vae_decoder_stem: null pointer");
    if (latents_bf16 != 0 && latents_bf16 != 1) return fail(GD_NN_ERR_INVALID_ARG, "vae_decoder_stem: latents_bf16 must be 0 or 1");
    if (!gd_nn_vae_decoder_stem_supported(N, h, w, Cout))
        return fail(GD_NN_ERR_INVALID_ARG, "vae_decoder_stem: needs N in [1, 65535], h, w >= 1, Cout % 64 == 0 in [64, 512] "
                                           "and N*h*w*Cout < 2^31");
    const dim3 grid((unsigned)((w + ST_T - 1) / ST_T), (unsigned)((h + ST_T - 1) / ST_T), (unsigned)N);
    if (latents_bf16)
        hipLaunchKernelGGL(stem_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, latents, inv_scale,
                           (const uint16_t*)pq_weight, (const uint16_t*)pq_bias, (const uint16_t*)weight,
                           (const uint16_t*)bias, (uint16_t*)y, h, w, Cout);
    else
        hipLaunchKernelGGL(stem_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, latents, inv_scale,
                           (const uint16_t*)pq_weight, (const uint16_t*)pq_bias, (const uint16_t*)weight,
                           (const uint16_t*)bias, (uint16_t*)y, h, w, Cout);
    return launch_status("vae_decoder_stem: launch failed");
}

int gd_nn_vae_decoder_head_supported(int N, int H, int W, int C, int G)
{
    if (N < 1 || H < 1 || W < 1 || N > 65535) return 0;
    if (C < 64 || C > HD_MAX_C || C % 64) return 0;
    if (G < 1 || C % G) return 0;
    if ((int64_t)N * H * W * C >= I31) return 0;
    return 1;
}

int gd_nn_vae_decoder_head(void* stream, const void* x, const float* mean_rstd, const void* gamma, const void* beta, int G,
                           const void* weight, const void* bias, void* out, int mode, int N, int H, int W, int C)
{
    if (!x || !mean_rstd || !gamma || !beta || !weight || !out)
        return fail(GD_NN_ERR_INVALID_ARG, "vae_decoder_head: null pointer");
    if (mode != GD_NN_VAE_HEAD_RAW && mode != GD_NN_VAE_HEAD_IMAGE)
        return fail(GD_NN_ERR_INVALID_ARG, "vae_decoder_head: mode must be GD_NN_VAE_HEAD_RAW or GD_NN_VAE_HEAD_IMAGE");
    if (!gd_nn_vae_decoder_head_supported(N, H, W, C, G))
        return fail(GD_NN_ERR_INVALID_ARG, "vae_decoder_head: needs N in [1, 65535], H, W >= 1, C % 64 == 0 in [64, 256], "
                                           "C % G == 0 and N*H*W*C < 2^31");
    const dim3 grid((unsigned)((W + HD_T - 1) / HD_T), (unsigned)((H + HD_T - 1) / HD_T), (unsigned)N);
    if (mode == GD_NN_VAE_HEAD_RAW)
        hipLaunchKernelGGL(head_kernel<GD_NN_VAE_HEAD_RAW>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x,
                           mean_rstd, (const uint16_t*)gamma, (const uint16_t*)beta, G, (const uint16_t*)weight,
                           (const uint16_t*)bias, out, H, W, C);
    else
        hipLaunchKernelGGL(head_kernel<GD_NN_VAE_HEAD_IMAGE>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)x,
                           mean_rstd, (const uint16_t*)gamma, (const uint16_t*)beta, G, (const uint16_t*)weight,
                           (const uint16_t*)bias, out, H, W, C);
    return launch_status("vae_decoder_head: launch failed");
}

const char* gd_nn_vae_decoder_last_error(void) { return g_err; }

}  // extern "C"
