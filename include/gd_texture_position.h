/*
 * gd_texture_position.h -- C-ABI and DEFINITION of the texture field's gradient to the sample POSITIONS: dL/dx of the
 * hash-grid encoding of include/gd_texture.h, what tiny-cuda-nn hands the reference's Renderer when the geometry moves
 * (fix_geo: false, Garment_Deformer_NeTF/netf/render/mesh_renderer.py:349-375).  Exported by libgd_raster.so (the kernels
 * and the entries: csrc/raster_texture.hip).  An opt-in addition: the entries of gd_texture.h and gd_texture_sorted.h stay
 * as they are.  Everything gd_texture.h defines (layout, encoding, field, backward formulas, the contract of the entries,
 * the error channel gd_texture_last_error) holds here; this header adds dx.
 *
 * DEFINITION.  In the notation of gd_texture.h: u_d = (x_d + 1) * 0.5, per level p_d = s_l u_d + 0.5, the cell c_d =
 * floor(p_d) and w_d = p_d - floor(p_d) EXACTLY as the forward forms them (same operations, same roundings).  Inside a cell
 * enc is trilinear in w, dw_d / dx_d = 0.5 s_l, and floor passes no gradient, so for a point that takes part
 *     dx_d = sum over l of (0.5 s_l) * sum_{i=0..7} sigma_d(i) * (prod_{k != d} wt_k(i)) * (denc[2l] g_i.x + denc[2l+1] g_i.y)
 * with sigma_d(i) = +1 if bit d of i is set, else -1; wt_k(i) = w_k if bit k of i is set, else 1 - w_k; g_i the grid
 * entry (offset_l + idx_i) of corner i.  On a cell wall the derivative is the one of the cell the forward chose (w_d = 0:
 * the cell above the wall).  fp32, in the order written (the file is built with -ffp-contract=off):
 *     dx_d = +0.0f
 *   per level, ascending:
 *     S_d = +0.0f
 *     per corner i = 0..7, ascending:
 *       t   = denc[2l] * g_i.x + denc[2l+1] * g_i.y                 (two products, one add)
 *       q_0 = wt_1(i) * wt_2(i),  q_1 = wt_0(i) * wt_2(i),  q_2 = wt_0(i) * wt_1(i)
 *       S_d = S_d + q_d * t    if bit d of i is set,     S_d = S_d - q_d * t    otherwise
 *     dx_d = dx_d + (0.5f * s_l) * S_d
 * A point with mask == 0 or a non-finite coordinate has dx = 0.  dx [N][3] is WRITTEN, every element, not added to: one
 * row per point, no atomics, so it is a pure function of (x, mask, grid, denc, layout) and reruns are bit-identical.  In
 * the fused entries denc is the W1^T dh the field's backward forms in registers (fused multiply-adds, not part of a
 * bit-exact statement, as in gd_texture.h); from denc on the operations are the ones above.
 *
 * WHAT THE FUSED ENTRIES LEAVE AS IT WAS.  dgrid, dw1, db1, dw2, db2 (and denc of the sorted entry) are what the entry
 * without dx gives: the MLP gradients and the sorted dgrid bit for bit, the atomic dgrid up to its order of arrival.  A
 * corner's grid entry is gathered once, in the loop that scatters (or would scatter) its dgrid contribution.
 *
 * Validation, N == 0 and the return codes are those of gd_texture.h; dx must not be null.  Scratch: the queries of
 * gd_texture.h / gd_texture_sorted.h (gd_texture_field_backward_scratch_bytes, gd_texture_sorted_scratch_bytes).
 */
#ifndef GD_TEXTURE_POSITION_H_INCLUDED
#define GD_TEXTURE_POSITION_H_INCLUDED

#include "gd_texture_sorted.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The encoding's gradient to the positions on its own.  grid: float [offset_L][F], 8-byte aligned; denc: float [N][L F];
 * dx: float [N][3], OUT.  One launch: one thread per point, eight float2 gathers per level. */
int gd_texture_encode_backward_pos(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                                   gd_texture_layout layout, const float* denc, float* dx);

/* gd_texture_field_backward plus dx [N][3] (OUT) in the same pass.  scratch: gd_texture_field_backward_scratch_bytes(N). */
int gd_texture_field_backward_pos(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                                  gd_texture_layout layout, const float* w1, const float* b1, const float* w2,
                                  const float* b2, const float* color, const float* dcolor, float* dgrid, float* dw1,
                                  float* db1, float* dw2, float* db2, float* dx, void* scratch);

/* gd_texture_field_backward_sorted plus dx [N][3] (OUT), written by the pass that stores denc. */
int gd_texture_field_backward_sorted_pos(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                                         gd_texture_layout layout, const float* w1, const float* b1, const float* w2,
                                         const float* b2, const float* color, const float* dcolor, float* dgrid,
                                         float* dw1, float* db1, float* dw2, float* db2, float* denc, float* dx,
                                         void* slab_scratch, void* sort_scratch);

#ifdef __cplusplus
}
#endif
#endif
