/*
 * gd_texture_sorted.h -- C-ABI and DEFINITION of the texture field's bit-reproducible grid gradient: dgrid by a stable
 * sort of the contributions by destination and one sequential sum per destination (csrc/raster_texture_sorted.hip, the
 * entries in csrc/raster_texture.hip; exported by libgd_raster.so).  An opt-in alternative to the atomic accumulation of
 * gd_texture_encode_backward / gd_texture_field_backward (include/gd_texture.h), which stay as they are and stay the
 * default.  Everything gd_texture.h defines (layout, encoding, field, backward formulas, the contract of the entries, the
 * error channel gd_texture_last_error) holds here; this header adds the ORDER of the sum.
 *
 * DEFINITION.  For each level l an ITEM is (n, i): point n = 0..N-1, corner i = 0..7, for the points that take part only
 * (mask != 0 and every coordinate finite, as in gd_texture.h).  The item's ENTRY is e = offset_l + idx_i and its
 * CONTRIBUTION is c_f = weight_i * denc[n][l F + f], f = 0..F-1: gd_texture.h's idx_i and weight_i, fp32, the product
 * rounded on its own (the files are built with -ffp-contract=off).  For every entry that has at least one item:
 *     s_f = +0.0f
 *     s_f = s_f + c_f     over the entry's items in ASCENDING (n, i), one fp32 add each
 *     dgrid[e F + f] = dgrid[e F + f] + s_f                   one add (.grad semantics)
 * An entry with no item is NOT WRITTEN: its bits, the sign of a zero included, stay.  Two corners of one point may share
 * an entry (res_l = 1, 2; hash collisions); they are added in the order of i.  This is the order a stable sort of the items
 * by entry produces, and it makes dgrid a pure function of (x, mask, denc, layout, dgrid before the call): reruns,
 * another stream, another device of the same kind give the same bits.  There is no tree and no blocked sum anywhere.  The
 * order is by point index: another N, or the same points permuted, is another sum.
 *
 * HOW.  Levels are handled in groups of at most 4 (the level on blockIdx.y).  Per group: one pass writes the key
 * idx_i of item 8 n + i at position 8 n + i (a point that takes no part gets the key size_l, which sorts last and is
 * never summed); a stable LSD radix sort of (key, item) with 8-bit digits, ceil(bit_length(size_l) / 8) passes per level,
 * each pass a histogram per 2 048-item tile, a scan per digit and a scatter that ranks by ballot in (wave, step, lane)
 * order; one pass writes the contributions in sorted order; one pass in which the first position of each entry adds its
 * contiguous run in order and adds the sum to dgrid with plain loads and stores.  No atomics on floats, no count is read
 * back, nothing waits for the device.
 *
 * LIMITS.  0 <= N <= 2^24 (the item id 8 n + i stays below 2^27 and the scratch grows with N): above that -1, with a
 * message that says to use the atomic path or to split the batch.  Scratch: gd_texture_sorted_scratch_bytes(N, layout)
 * <= 4096 N + 64 MiB, caller-owned, contents undefined before and after.  The MLP gradients of the fused entry are those
 * of gd_texture_field_backward bit for bit (same slab, same fixed-order sum).
 */
#ifndef GD_TEXTURE_SORTED_H_INCLUDED
#define GD_TEXTURE_SORTED_H_INCLUDED

#include "gd_texture.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device scratch the two entries below need at N points, non-decreasing in N; 0 for N <= 0 or an inconsistent
 * layout */
size_t gd_texture_sorted_scratch_bytes(int N, gd_texture_layout layout);

/* gd_texture_encode_backward with the sum above.  denc: float [N][L F]; dgrid: float [offset_L][F], added to. */
int gd_texture_encode_backward_sorted(void* stream, int N, const float* x, const uint8_t* mask, const float* denc,
                                      gd_texture_layout layout, float* dgrid, void* scratch);

/* gd_texture_field_backward with the sum above.  denc: float [N][32], 16-byte aligned, OUT: every element written, the
 * gradient to the encoding that was scattered (zeros for a point that takes no part): dgrid is the definition above
 * applied to exactly these values.  slab_scratch: gd_texture_field_backward_scratch_bytes(N); sort_scratch:
 * gd_texture_sorted_scratch_bytes(N, layout). */
int gd_texture_field_backward_sorted(void* stream, int N, const float* x, const uint8_t* mask, const float* grid,
                                     gd_texture_layout layout, const float* w1, const float* b1, const float* w2,
                                     const float* b2, const float* color, const float* dcolor, float* dgrid, float* dw1,
                                     float* db1, float* dw2, float* db2, float* denc, void* slab_scratch,
                                     void* sort_scratch);

#ifdef __cplusplus
}
#endif
#endif
