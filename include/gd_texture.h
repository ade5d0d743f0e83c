/*
 * gd_texture.h -- C-ABI and DEFINITIONS of the NeTF stage's texture field (stage 4 of the reference:
 * Garment_Deformer_NeTF/netf/render/texture_encoder.py:8-37 and mesh_renderer.py:368-375), exported by libgd_raster.so
 * (csrc/raster_texture.hip): a multiresolution hash-grid encoding of 3-D points with its gradient to the grid, and the
 * fused field  color = sigmoid(mlp(encode(x)))  with the gradients to the grid and to the MLP.
 *
 * Same contract as gd_mesh.h: plain device pointers, caller's HIP stream, caller-owned scratch with a *_scratch_bytes
 * query, no host synchronisation, every forward output element written.  Every entry validates its arguments before any
 * device work: a null pointer (mask may be null: every point counts), N < 0 or N > 2^30, a grid that is not 8-byte
 * aligned or an inconsistent layout returns -1 with a message in gd_texture_last_error().  N == 0 returns 0 and launches
 * nothing.  Return 0 on success, -1 on a bad call, -2 on a HIP error.
 *
 * LAYOUT.  D = 3 input dimensions, F = 2 features per level, L levels (1 <= L <= 16), at most 2^log2_T entries per level
 * (log2_T <= 24), base resolution N0, per-level scale b.  The layout is computed once on the host in float64
 * (texture_field.grid_layout) and handed over by value; no device or libm transcendental takes part.  For level l:
 *     s_l      = (float)(2^(l log2 b) N0 - 1)
 *     res_l    = ceil(s_l) + 1
 *     size_l   = min(round_up(res_l^3, 8), 2^log2_T)          entries
 *     offset_l = size_0 + ... + size_{l-1},   offset_0 = 0;   offset_L is the number of entries
 * A level is DENSE iff res_l^3 <= size_l, otherwise HASHED.  The parameters are one flat fp32 array [offset_L * F],
 * ordered level, entry, feature.  A layout is consistent iff 1 <= L <= 16, every res is in 1..2^21, every size > 0 and
 * offset_0 = 0, offset_{l+1} = offset_l + size_l, offset_L <= 2^28 (so that no index leaves the array).
 *
 * ENCODING of a point x in R^3.  fp32, in the order written (the file is built with -ffp-contract=off):
 *     u_d = (x_d + 1) * 0.5                                   (the reference's (x + bound) / (2 bound), bound = 1)
 *   per level:
 *     p_d = s_l * u_d, then p_d = p_d + 0.5                   (two roundings)
 *     c_d = (uint32)(int32)floor(p_d),  w_d = p_d - floor(p_d)    (|p_d| < 2^31; beyond that the conversion saturates)
 *     corner i = 0..7:  delta_d = bit d of i,  g_d = c_d + delta_d               (uint32, wrap-around)
 *                       weight_i = ((delta_0 ? w_0 : 1 - w_0) * (delta_1 ? w_1 : 1 - w_1)) * (delta_2 ? w_2 : 1 - w_2)
 *                       dense:   idx_i = (g_0 + g_1 res + g_2 res res) mod size_l            (uint32, wrap-around)
 *                       hashed:  idx_i = (g_0 ^ g_1 2654435761 ^ g_2 805459861) mod size_l   (uint32, wrap-around)
 *     enc[l F + f] = sum over i = 0..7, ascending from 0, of weight_i * grid[(offset_l + idx_i) F + f]
 * Nothing is clamped: the mod keeps every index inside its level for any x, points outside [-1, 1] included; the values
 * above are defined where every |p_d| < 2^31 (|x| below about 4e6 at the production scales); beyond that c_d is whatever
 * the saturating conversion gives and w_d may be NaN (p_d = inf), so the output may be non-finite, never out of range.  A
 * point with a non-finite coordinate, or with mask == 0, has output 0 and contributes to no gradient.  Interpolation is
 * linear; smoothstep is not built (the reference never asks for it).
 *
 * FIELD (needs L F = 32).  W1 [32][32] and W2 [3][32] in nn.Linear layout (row = output), fp32:
 *     h = relu(W1 enc + b1),  o = W2 h + b2,  color = sigmoid(o) = 1 / (1 + exp(-o))
 * The two matrix products are fused multiply-adds from the bias upwards in ascending column order; they are not part of
 * the bit-exact statement, the encoding is.
 *
 * BACKWARD.  From dcolor [N][3]:  do = dcolor color (1 - color);  dW2 += do (x) h,  db2 += do;  dh = W2^T do where
 * h > 0, else 0;  dW1 += dh (x) enc,  db1 += dh;  denc = W1^T dh;
 *     dgrid[(offset_l + idx_i) F + f] += weight_i * denc[l F + f]
 * enc and h are recomputed, the forward saves color only.  EVERY gradient is ADDED to the caller's buffer (.grad
 * semantics: the buffers may be views of an optimizer's flat gradient buffer).  There is no gradient to x.
 *
 * DETERMINISM.  The forward is bit-reproducible.  The four MLP gradients are summed in a fixed order: a workgroup adds
 * its points in ascending order, writes one row of partials to the scratch slab, and one pass adds the rows in ascending
 * order to the destination; reruns are bit-identical.  dgrid is accumulated with no-return fp32 atomicAdd, as
 * tiny-cuda-nn does: its last bits depend on the order of arrival and differ from run to run.  These entries stay as they
 * are and stay the default; gd_texture_sorted.h declares the opt-in entries whose dgrid is a pure function of the inputs
 * (a stable sort of the contributions by entry, then one sequential sum per entry in ascending (point, corner) order).
 */
#ifndef GD_TEXTURE_H_INCLUDED
#define GD_TEXTURE_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_TEXTURE_MAX_LEVELS 16
#define GD_TEXTURE_FEATURES 2       /* F */
#define GD_TEXTURE_FIELD_WIDTH 32   /* L F of the fused path, and the hidden width */

typedef struct gd_texture_layout {
    int32_t num_levels;                         /* L */
    float scale[GD_TEXTURE_MAX_LEVELS];         /* s_l */
    int32_t res[GD_TEXTURE_MAX_LEVELS];         /* res_l */
    int32_t size[GD_TEXTURE_MAX_LEVELS];        /* size_l, entries */
    int32_t offset[GD_TEXTURE_MAX_LEVELS + 1];  /* offset_l, entries; offset[L] = total */
} gd_texture_layout;

/* x: float [N][3]; mask: uint8 [N] or NULL; grid: float [offset_L][F]; enc: float [N][L F].  One launch. */
int gd_texture_encode_forward(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                              gd_texture_layout layout, float* enc);

/* denc: float [N][L F]; dgrid: float [offset_L][F], added to.  One launch. */
int gd_texture_encode_backward(void* stream, int N, const float* x, const uint8_t* mask, const float* denc,
                               gd_texture_layout layout, float* dgrid);

/* color: float [N][3].  One launch. */
int gd_texture_field_forward(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                             gd_texture_layout layout, const float* w1, const float* b1, const float* w2,
                             const float* b2, float* color);

/* bytes of device scratch gd_texture_field_backward needs: the slab of per-workgroup partials (0 for N <= 0) */
size_t gd_texture_field_backward_scratch_bytes(int N);

/* color: what the forward returned for these inputs; dcolor: float [N][3]; dgrid, dw1 [32][32], db1 [32], dw2 [3][32],
 * db2 [3]: added to.  Two launches: the points, then the fixed-order sum of the slab. */
int gd_texture_field_backward(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                              gd_texture_layout layout, const float* w1, const float* b1, const float* w2,
                              const float* b2, const float* color, const float* dcolor, float* dgrid, float* dw1,
                              float* db1, float* dw2, float* db2, void* scratch);

const char* gd_texture_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
