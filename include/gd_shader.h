/*
 * gd_shader.h -- NORMATIVE DEFINITION of the arithmetic of the neural shader and the shading loss of the mesh deformer's
 * second stage (stage 3 of the reference: Garment_Deformer_NeTF/deformer/modules/neuralshader.py, fc.py, embedder.py and
 * deformer/losses/shading.py) for an implementation on the bf16 matrix cores.  No such implementation is built yet: this
 * header declares no entry and libgd_raster.so exports none.  What it holds is what a kernel and its tests must agree on --
 * the layer table, the padded and packed layouts, the rounding points, and the integer mix of the sampling as C that
 * compiles on the host and on the device.  tests/shader_reference.py restates all of it in torch and numpy;
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

#endif
