/*
 * gd_views.h -- C-ABI and DEFINITIONS of reading the captured views: the row unfilter of inflated 8-bit PNG streams and
 * the unpacking of a view's byte images into the float images the deformer (Garment_Deformer_NeTF/deformer/core/view.py,
 * View.load) and the texture fit (netf/view_core/view.py) work on, exported by libgd_raster.so (csrc/raster_views.hip).
 * garmentdreamer_amd/views.py drives the entries; tests/views_reference.py states them in numpy.
 *
 * Same contract as gd_fit.h: plain device pointers, the caller's HIP stream as the first argument, no host
 * synchronisation inside any entry, every output element written, integers only in the unfilter and no atomics anywhere,
 * reruns bit-identical.  Every entry validates its arguments before any device work: a null pointer, a size below 1 or
 * above GD_VIEWS_MAX_SIDE, bpp or rgb_channels outside {3, 4} or a misaligned pointer returns -1 with a message in
 * gd_mesh_last_error().  Return 0 on success, -1 on a bad call, -2 on a HIP error.  Built with -ffp-contract=off: every
 * fp32 operation below is one IEEE rounding.
 *
 * ---- 1. UNFILTER -----------------------------------------------------------------------------------------------------
 * filtered: B inflated streams of equal geometry, one after the other: each H rows of 1 + W bpp bytes, the row's filter
 * type first.  out: uint8 [B][H][W][bpp].  With i the byte index within a row, all arithmetic mod 256:
 *     recon(r, i) = filt(r, i) + pred(a, b, c),   a = recon(r, i - bpp),  b = recon(r - 1, i),  c = recon(r - 1, i - bpp),
 * neighbours outside the image are 0, and pred by the row's type is
 *     0 none: 0      1 sub: a      2 up: b      3 average: (a + b) >> 1 (the sum not reduced mod 256)      4 Paeth:
 *     p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|; a if pa <= pb and pa <= pc, else b if pb <= pc, else c.
 * A type byte above 4 is treated as 0; the host refuses such a stream before it is uploaded.  Every loop of the kernel is
 * bounded by H, W and bpp alone: no stream can make it spin.  filtered and out must be 4-byte aligned.
 *
 * ---- 2. UNPACK -------------------------------------------------------------------------------------------------------
 * x(byte) = fl((float) byte / 255.0f).  Of the view's normal image normal_rgba uint8 [H][W][4] and its colour image
 * rgb uint8 [H][W][rgb_channels]:
 *     mask   [H][W][1] = x(alpha of normal_rgba)
 *     normal [H][W][3]: n = fl(fl(x 2) - 1);  n_y = fl(n_y -1);  normal = fl(fl(n + 1) / 2)
 *     rgb_out[H][W][3] = x of the first three channels of rgb
 * (View.load's ``n*2-1; n[...,1]*=-1; (n+1)/2``).  unpack_rgba is the texture fit's: rgb_out and mask of one RGBA image.
 * All images must be 16-byte aligned.
 */
#ifndef GD_VIEWS_H_INCLUDED
#define GD_VIEWS_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_VIEWS_MAX_SIDE 8192     /* H, W and B */
#define GD_VIEWS_BAND_ROWS 64      /* rows of a band: one per lane of the wave that owns the image */
#define GD_VIEWS_CHUNK_PIXELS 64   /* pixels of a row chunk staged through LDS */
#define GD_VIEWS_PIXELS_PER_LANE 4 /* of the unpack kernels */

int gd_views_png_unfilter(void* stream, const uint8_t* filtered, uint8_t* out, int B, int H, int W, int bpp);

int gd_views_unpack(void* stream, const uint8_t* normal_rgba, const uint8_t* rgb, int rgb_channels, float* normal,
                    float* mask, float* rgb_out, int H, int W);

int gd_views_unpack_rgba(void* stream, const uint8_t* rgba, float* rgb_out, float* mask, int H, int W);

#ifdef __cplusplus
}
#endif
#endif
