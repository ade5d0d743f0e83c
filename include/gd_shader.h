/*
 * gd_shader.h -- NORMATIVE DEFINITION of the arithmetic of the neural shader and the shading loss of the mesh deformer's
 * second stage (stage 3 of the reference: Garment_Deformer_NeTF/deformer/modules/neuralshader.py, fc.py, embedder.py and
 * deformer/losses/shading.py) for an implementation on the bf16 matrix cores, and the C-ABI of that
 * implementation in libgd_raster.so (csrc/raster_shader.hip: selection, features, pack, L1 and feature backward in fp32;
 * csrc/raster_shader_mfma.hip: the eight products forward, towards the input and towards the weights).  It holds what the
 * kernels and their tests agree on -- the layer table, the padded and packed layouts, the rounding points, the integer mix
 * of the sampling as C that compiles on the host and on the device -- then the layouts of the buffers that cross the ABI
 * and the entries (below the inline functions).  tests/shader_reference.py restates all of it in torch and numpy;
 * tests/test_shader_cpu.py compiles this header and compares hash32, the threshold and the layout tables bit for bit.
 *
 * THE NETWORK.  NeuralShader(hidden_features_size=256, hidden_features_layers=3, fourier_features='positional',
 * fft_scale=4, activation='relu', last_activation=Sigmoid): eight linear layers l = 0 .. 7,
 *      l      0    1    2    3    4    5    6    7
 *      in    27  256  256  256  256  262  128  128        (K_l;  padded Kp_l: 32 256 256 256 256 288 128 128)
 *      out  256  256  256  256  256  128  128    3        (O_l;  padded Op_l: 256 256 256 256 256 128 128 32)
 *      ReLU yes  yes  yes  yes   no  yes  yes   no
 * layers 0..4 are `diffuse`, 5..7 `specular`; colour = sigmoid(logits), logits the output of layer 7.
 *   feat[32]  = enc(p) = [p, sin(1p), cos(1p), sin(2p), cos(2p), sin(4p), cos(4p), sin(8p), cos(8p)] (27 values; the frequency
 *               is the outer loop, sin before cos, each 3 wide), then 5 zeros
 *   extra[32] = [normal(3), view_dir(3)], then 26 zeros;  the input of layer 5 is [h(256), extra(32)], h the output of layer 4
 * Master weights are float [O_l][K_l] (nn.Linear), biases float [O_l].
 *
 * PACKING.  The weights are rounded to bf16 (round to nearest even, as every rounding here) into W_l as [Op_l][Kp_l] for
 * l = 0..7 one after the other, zeros in the padding: W_l starts at gd_shader_packed_offset(l) halves,
 * GD_SHADER_PACKED_ELEMS = 327 680 halves (640 KB) in all.
 *
 * ROUNDING POINTS.  The same whether a layer is its own launch or part of a fused kernel:
 *   feat, extra -> bf16;   Y_l = bf16(act_l(acc_l + b_l)), acc_l the fp32 sum over k of the bf16 products X_l[n][k] W_l[o][k],
 *   b_l in fp32, act_l ReLU or the identity;  X_{l+1} = Y_l;  logits = acc_7 + b_7 stay fp32.
 *   backward: dlogits -> bf16 (dZ_7);  dZ_{l-1} = bf16([Y_{l-1} > 0] sum_o dZ_l[n][o] W_l[o][k]) for the layers with a ReLU,
 *   without the mask into h (l = 5, k < 256);  dextra = the columns k >= 256 of layer 5's product and dfeat = layer 0's
 *   product stay fp32;  dW_l[o][k] = sum_n dZ_l[n][o] X_l[n][k],  db_l[o] = sum_n dZ_l[n][o], fp32, summed over the points in
 *   an order that depends only on the number of points and the launch geometry; no floating-point atomics.
 *
 * FEATURES (fp32, in the order written).
 *   enc as above with sinf / cosf of (float)f * p_c;  v = center - p, l = |v|, u = v / max(l, 1e-12) (|.| and dot as
 *   gd_mesh_losses.h);  view_dir = u.
 *   backward:  dp_c = dfeat[c] + sum over f = 1, 2, 4, 8 in that order of f (cos(f p_c) dfeat[s_f + c] - sin(f p_c) dfeat[s_f + 3 + c]),
 *   s_f the index of sin(f p);  g_u = dextra[3..5];  g_v = l > 1e-12 ? (g_u - u dot(u, g_u)) / l : g_u / 1e-12;
 *   dposition = dp - g_v;  dnormal = dextra[0..2].
 *
 * SELECTION.  Pixel i = y W + x is valid when view_mask > 0, mask > 0 and cos_1e-6(d, n_cam) <= 0 (gd_mesh_losses.h, SHARED).
 * A valid pixel is kept when p >= 1 or gd_shader_hash32(seed, step, i) < gd_shader_keep_threshold(p) = floor(p 2^32).  The
 * kept pixels are taken in ascending order; beyond a capacity they are dropped in pixel order and counted.  The reference
 * keeps exactly int(n p) pixels drawn by the host's RNG; here the number kept is binomial -- a stated deviation.
 *
 * LOSS.  c = 1 / (1 + expf(-logit));  term_n = (|c_0 - t_0| + |c_1 - t_1|) + |c_2 - t_2| with t the pixel of rgb;
 * loss = sum / (3 (float)count), 0 with exact-zero gradients when count = 0 (the reference: NaN);
 * dlogit_c = sign(c_c - t_c) ((dloss / (3 (float)count)) (c_c (1 - c_c))), sign(0) = 0.
 */
#ifndef GD_SHADER_H_INCLUDED
#define GD_SHADER_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#define GD_SHADER_LAYERS 8
#define GD_SHADER_PACKED_ELEMS 327680
#define GD_SHADER_FEATURES 32 /* enc (27) padded */
#define GD_SHADER_EXTRA 32    /* normal, view_dir (6) padded */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GD_SHADER_INLINE static inline __host__ __device__
#else
#define GD_SHADER_INLINE static inline
#endif

/* K_l, Kp_l, O_l, Op_l and whether a ReLU follows layer l */
GD_SHADER_INLINE int gd_shader_in(int l, int padded)
{
    return l == 0 ? (padded ? 32 : 27) : l < 5 ? 256 : l == 5 ? (padded ? 288 : 262) : 128;
}
GD_SHADER_INLINE int gd_shader_out(int l, int padded) { return l < 5 ? 256 : l < 7 ? 128 : (padded ? 32 : 3); }
GD_SHADER_INLINE int gd_shader_relu(int l) { return l != 4 && l != 7; }

/* first half of W_l in the packed buffer; gd_shader_packed_offset(GD_SHADER_LAYERS) == GD_SHADER_PACKED_ELEMS */
GD_SHADER_INLINE size_t gd_shader_packed_offset(int l)
{
    size_t off = 0;
    int i;
    for (i = 0; i < l; i++) off += (size_t)gd_shader_out(i, 1) * (size_t)gd_shader_in(i, 1);
    return off;
}

/* the integer mix of the sampling: uint32, wrapping */
GD_SHADER_INLINE uint32_t gd_shader_hash32(uint32_t seed, uint32_t step, uint32_t pixel)
{
    uint32_t x = pixel ^ (seed * 0x9E3779B1u) ^ (step * 0x85EBCA77u);
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

/* floor(p 2^32) for 0 <= p < 1; a caller keeps every valid pixel without asking when p >= 1 */
GD_SHADER_INLINE uint32_t gd_shader_keep_threshold(float p) { return (uint32_t)((double)p * 4294967296.0); }

/* ---- BUFFERS THAT CROSS THE ABI ---------------------------------------------------------------------------------------
 * Everything is sized from `capacity` (the most points a call may keep), never from the number kept, which lives on the
 * device.  rows = gd_shader_rows(capacity): capacity rounded up to the 128-point tile of the product kernels.
 *   index     int32 [capacity]   the kept pixels in ascending order; entries at or past count are not written
 *   counters  int32 [4]          {count, dropped, count + dropped, 0}: count = min(kept, capacity)
 *   act       bf16, gd_shader_act_elems(rows) halves: X_l as [rows][Kp_l] for l = 0..7 one after the other, X_l at
 *             gd_shader_act_offset(l, rows).  X_0 = feat; X_5 = [h(256), extra(32)]: layer 4 writes the first 256 columns
 *             of its 288-wide rows, the features kernel the last 32.  Rows count .. rows of X_0 and of extra are ZERO; a
 *             tile of 128 rows that starts at or past count is neither computed nor read (its rows may hold anything), a
 *             partly filled tile computes act(b) in its rows past count.   3200 bytes per point.
 *   logits    float [rows][3]
 *   dz        bf16, gd_shader_dz_elems(rows) halves: dZ_l as [rows][Op_l], at gd_shader_dz_offset(l, rows).  dZ_7 has its
 *             three columns and 29 zeros; rows count .. rows of dZ_7 are ZERO, so every later dZ of a partly filled tile is.
 *             3136 bytes per point.
 *   dfeat, dextra   float [rows][32]: layer 0's input gradient, and the columns 256.. of layer 5's
 *   params, grad    float [GD_SHADER_PARAM_ELEMS]: weight [O_l][K_l] at gd_shader_param_offset(l, 0), bias [O_l] at
 *             gd_shader_param_offset(l, 1), each tensor at a multiple of 64 floats, layer by layer, weight then bias
 *   packed, packed_t  bf16 [GD_SHADER_PACKED_ELEMS]: W_l [Op_l][Kp_l], and its transpose [Kp_l][Op_l], both at
 *             gd_shader_packed_offset(l)
 *   scratch   gd_shader_scratch_bytes(capacity) bytes: the L1's partial sums, float [rows / 256], then the weight
 *             gradient's: float [slabs][Op_l Kp_l + Op_l] of the layer in flight, slab s holding the sums over the rows
 *             s S .. s S + S - 1, S = gd_shader_slab_rows(rows), slabs = ceil(rows / S) <= GD_SHADER_MAX_SLABS
 *   select scratch   gd_shader_select_scratch_bytes(pixels): int32 [2][ceil(pixels / 256)] (counts, their exclusive scan)
 * SUMS.  The L1 as gd_mesh_losses.h SUMS over rows instead of pixels.  A weight gradient: inside a slab the matrix cores add
 * the points in ascending chunks of 16; slabs that start below count are then added in ascending order from 0 and the
 * result is ADDED to grad.  The bias gradient is the same product against a column of ones.  */
#define GD_SHADER_TILE_ROWS 128
#define GD_SHADER_MAX_SLABS 64
#define GD_SHADER_PARAM_ELEMS 320960
#define GD_SHADER_ACT_WIDTH 1600
#define GD_SHADER_DZ_WIDTH 1568

GD_SHADER_INLINE int64_t gd_shader_rows(int64_t capacity)
{
    return (capacity + GD_SHADER_TILE_ROWS - 1) / GD_SHADER_TILE_ROWS * GD_SHADER_TILE_ROWS;
}
GD_SHADER_INLINE size_t gd_shader_act_offset(int l, int64_t rows)
{
    size_t off = 0;
    int i;
    for (i = 0; i < l; i++) off += (size_t)rows * (size_t)gd_shader_in(i, 1);
    return off;
}
GD_SHADER_INLINE size_t gd_shader_act_elems(int64_t rows) { return gd_shader_act_offset(GD_SHADER_LAYERS, rows); }
GD_SHADER_INLINE size_t gd_shader_dz_offset(int l, int64_t rows)
{
    size_t off = 0;
    int i;
    for (i = 0; i < l; i++) off += (size_t)rows * (size_t)gd_shader_out(i, 1);
    return off;
}
GD_SHADER_INLINE size_t gd_shader_dz_elems(int64_t rows) { return gd_shader_dz_offset(GD_SHADER_LAYERS, rows); }
GD_SHADER_INLINE size_t gd_shader_param_offset(int l, int bias)
{
    size_t off = 0;
    int i;
    for (i = 0; i < l; i++)
        off += ((size_t)gd_shader_out(i, 0) * (size_t)gd_shader_in(i, 0) + 63) / 64 * 64 + ((size_t)gd_shader_out(i, 0) + 63) / 64 * 64;
    if (bias) off += ((size_t)gd_shader_out(l, 0) * (size_t)gd_shader_in(l, 0) + 63) / 64 * 64;
    return off;
}
GD_SHADER_INLINE int64_t gd_shader_slab_rows(int64_t rows)
{
    return gd_shader_rows((rows + GD_SHADER_MAX_SLABS - 1) / GD_SHADER_MAX_SLABS);
}

/* ---- ENTRIES ----------------------------------------------------------------------------------------------------------
 * The contract of gd_mesh_losses.h: plain device pointers, the caller's HIP stream, caller-owned scratch, no host
 * synchronisation, no floating-point atomics, no workgroup waits for another, reruns bit-identical.  Every entry validates
 * its arguments before any device work: a null pointer, a size that is not positive, H W >= 2^30, capacity < 1 or
 * > 2^24, a layer outside 0..7 or p < 0 returns -1 with a message in gd_mesh_last_error().  0 on success, -2 on a HIP
 * error.  Every launch is sized from capacity (or H W); the kernels read count from `counters`. */
#ifdef __cplusplus
extern "C" {
#endif

size_t gd_shader_select_scratch_bytes(int64_t pixels);
size_t gd_shader_scratch_bytes(int64_t capacity);

/* SELECTION: three launches (counts per 256 pixels, one workgroup scanning the counts, scatter).  camera as gd_mesh_losses.h. */
int gd_shader_select(void* stream, int H, int W, const float* normal, const float* position, const float* mask,
                     const float* view_mask, const float* camera, float p, uint32_t seed, uint32_t step, int64_t capacity,
                     int32_t* index, int32_t* counters, void* scratch);

/* FEATURES of the kept pixels into X_0 and the extra columns of X_5, zeros in the rows count .. rows. */
int gd_shader_features(void* stream, int H, int W, const float* position, const float* normal, const float* camera,
                       int64_t capacity, const int32_t* index, const int32_t* counters, void* act);
/* the same of N <= capacity given points [N][3] with their view directions; writes counters = {N, 0, N, 0} */
int gd_shader_features_points(void* stream, int64_t N, const float* position, const float* normal, const float* view_dir,
                              int64_t capacity, int32_t* counters, void* act);

/* PACK: params -> packed and packed_t, one launch */
int gd_shader_pack(void* stream, const float* params, void* packed, void* packed_t);

/* THE PRODUCTS of layer l, one tile kernel per kind.  forward: X_{l+1} (logits for l = 7) from X_l; backward_input:
 * dZ_{l-1} (dfeat for l = 0; dZ_4 and dextra for l = 5) from dZ_l; backward_weight: two launches, the slab sums and their
 * fixed-order sum added into grad. */
int gd_shader_forward_layer(void* stream, int l, int64_t capacity, const int32_t* counters, const void* packed,
                            const float* params, void* act, float* logits);
int gd_shader_backward_input_layer(void* stream, int l, int64_t capacity, const int32_t* counters, const void* packed_t,
                                   const void* act, void* dz, float* dfeat, float* dextra);
int gd_shader_backward_weight_layer(void* stream, int l, int64_t capacity, const int32_t* counters, const void* act,
                                    const void* dz, float* grad, void* scratch);

/* L1.  rgb [H][W][3]; loss: one float.  forward: two launches.  backward: dloss one float on the device; writes dZ_7 and,
 * unless NULL, the unrounded dlogits float [rows][3]. */
int gd_shader_l1_forward(void* stream, int H, int W, int64_t capacity, const int32_t* index, const int32_t* counters,
                         const float* logits, const float* rgb, float* loss, void* scratch);
int gd_shader_l1_backward(void* stream, int H, int W, int64_t capacity, const int32_t* index, const int32_t* counters,
                          const float* logits, const float* rgb, const float* dloss, void* dz, float* dlogits);
/* colour [N][3] = 1 / (1 + expf(-logits)) */
int gd_shader_colour(void* stream, int64_t N, const float* logits, float* colour);

/* FEATURE BACKWARD: dposition, dnormal [H][W][3], every pixel written, exact zeros where the pixel is not kept */
int gd_shader_features_backward(void* stream, int H, int W, const float* position, const float* camera, int64_t capacity,
                                const int32_t* index, const int32_t* counters, const float* dfeat, const float* dextra,
                                float* dposition, float* dnormal);

#ifdef __cplusplus
}
#endif

#endif
