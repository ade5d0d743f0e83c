/*
 * gd_bake.h -- C-ABI and DEFINITIONS of the texture bake's padding (the last step of stage 4 of the reference:
 * Renderer.export_mesh, Garment_Deformer_NeTF/netf/render/mesh_renderer.py:260-313, which calls kiui's uv_padding on the
 * host), exported by libgd_raster.so (csrc/raster_bake.hip): for every texel of a UV atlas the covered texel whose
 * colour it takes, and the gather that turns a float image into the 8-bit texture.
 *
 * Same contract as gd_mesh.h: plain device pointers, caller's HIP stream, no host synchronisation, every output element
 * written, no atomics, reruns bit-identical.  Every entry validates its arguments before any device work: a null
 * pointer, H < 1, W < 1, H W >= 2^31, padding outside 0..GD_BAKE_MAX_PADDING or C outside 1..GD_BAKE_MAX_CHANNELS
 * returns -1 with a message in gd_bake_last_error().  Return 0 on success, -1 on a bad call, -2 on a HIP error.
 *
 * PADDING INDEX.  Integers only.  mask is uint8 [H][W], nonzero = covered; texels outside the image are uncovered;
 * 0 <= p <= GD_BAKE_MAX_PADDING.  For texel (r, c):
 *     covered:                                                            src = r W + c
 *     uncovered, and no covered (r', c') has |r - r'| + |c - c'| <= p:    src = -1
 *     otherwise:   src = r' W + c' of the covered texel that minimises (r - r')^2 + (c - c')^2 over ALL covered texels;
 *                  among equals the lowest row-major index r' W + c' wins
 * p = 0 is the identity on covered texels and -1 elsewhere.
 *
 * Two facts a kernel may use:
 *   - the L1 distance bounds the Euclidean one from above, so a witness with |dr| + |dc| <= p has dr^2 + dc^2 <= p^2, the
 *     minimiser is no farther, and so it lies in the (2p+1)^2 window around the texel: only that window need be searched;
 *   - the minimiser of an uncovered texel has an uncovered 4-neighbour (the neighbour one step towards the texel is
 *     strictly nearer, so it cannot be covered): restricting the search to such boundary texels changes nothing.
 *
 * This is what kiui's uv_padding(image, mask, padding, backend='knn') is understood to compute: the region to fill is
 * binary_dilation(mask, iterations = padding) with the 4-connected element, minus the mask (the L1 ball), and each of
 * its texels takes one nearest neighbour among the mask's two outer layers; where two covered texels are equally near,
 * kiui takes whichever its KD-tree returns, this definition the lowest index.
 *
 * RESOLVE.  image is float [H][W][C], C <= 4; src is int32 [H][W]; out is uint8 [H][W][C]:
 *     0 <= src < H W:   out[t][k] = (uint8)(int)(clamp(image[src][k], 0, 1) * 255.0f)     (fp32 product, truncated)
 *     otherwise:        out[t][k] = 0
 * clamp(NaN) = 0.  A src outside [0, H W) is never followed.
 */
#ifndef GD_BAKE_H_INCLUDED
#define GD_BAKE_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_BAKE_MAX_PADDING 64
#define GD_BAKE_MAX_CHANNELS 4

/* mask: uint8 [H][W]; src: int32 [H][W], every element written.  One launch. */
int gd_bake_pad_index(void* stream, int H, int W, int padding, const uint8_t* mask, int32_t* src);

/* image: float [H][W][C]; src: int32 [H][W]; out: uint8 [H][W][C], every element written.  One launch. */
int gd_bake_resolve_u8(void* stream, int H, int W, int C, const float* image, const int32_t* src, uint8_t* out);

const char* gd_bake_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
