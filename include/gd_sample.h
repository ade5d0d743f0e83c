/*
 * gd_sample.h -- C-ABI of the texture sampling of the mesh path, exported by libgd_raster.so (csrc/raster_sample.hip):
 * what a textured render needs beyond include/gd_mesh.h.  Plain device pointers, caller's HIP stream, caller-owned
 * buffers, no torch types, no host synchronisation and nothing read back inside any entry, no float atomics, reruns
 * bit-identical.  Messages go through gd_mesh_last_error().
 *
 *   gd_sample_rast_db            <- the second output of nvdiffrast's rasterize (screen-space derivatives of u, v)
 *   gd_sample_interpolate_da     <- interpolate(..., rast_db=, diff_attrs='all'): the attributes' screen-space derivatives
 *   gd_sample_build_mips         <- the mip pyramid texture() builds
 *   gd_sample_texture_forward    <- texture(): nearest, linear, linear-mipmap-nearest, linear-mipmap-linear; wrap, clamp
 *   gd_sample_texture_items / _reduce / _fold    its gradient to the texture, by stable sort and sum
 *   (Garment_Deformer_NeTF/netf/render/mesh_renderer.py:46-58 is the chain the reference runs.)
 *
 * UNVERIFIED: nvdiffrast is not available to this project, so the agreement of these definitions with it has not been
 * measured.  The level rule is the one it publishes (the larger singular value of the uv Jacobian in level-0 texels);
 * the texel-centre convention, the wrap rule and the order of the fp32 operations are this header's own.
 * Not built: a gradient to uv or uv_da, the 'cube' and 'zero' boundary modes, a mip level bias.
 *
 * Everything below is fp32 with one rounding per operation in the stated order (the file is built without contraction).
 *
 * ---- rast_db ---------------------------------------------------------------------------------------------------------
 * One pass per pixel over a finished rast.  Pixel (r, c) with id t + 1 > 0: with fx, fy, q_i = (qx_i, qy_i), a0, a1, a2 of
 * gd_mesh.h ("gradients to vertex positions": the unsnapped u = a0 / s, v = a1 / s) and s = (a0 + a1) + a2,
 *     da0x = qy1 w2 - w1 qy2,  da1x = qy2 w0 - w2 qy0,  da2x = qy0 w1 - w0 qy1        (d a_i / d fx:  dq_i/dfx = (-w_i, 0))
 *     da0y = w1 qx2 - qx1 w2,  da1y = w2 qx0 - qx2 w0,  da2y = w0 qx1 - qx0 w1        (d a_i / d fy:  dq_i/dfy = (0, -w_i))
 *     dsx = (da0x + da1x) + da2x, dsy likewise;   ss = s s
 *     ux = (da0x s - a0 dsx) / ss,  uy = (da0y s - a0 dsy) / ss,  vx = (da1x s - a1 dsx) / ss,  vy = (da1y s - a1 dsy) / ss
 *     rast_db[r][c] = (ux kx, uy ky, vx kx, vy ky)  with kx = 2 / float(W), ky = 2 / float(H)
 * i.e. (du/dX, du/dY, dv/dX, dv/dY) per pixel step; the row index grows with y_ndc.  All four are 0 on background, for
 * an id or a vertex index out of range, and where s is 0 or not finite.
 *
 * ---- attribute derivatives -------------------------------------------------------------------------------------------
 * With a_i = attr[tri[id][i]]:  e0 = a0[k] - a2[k], e1 = a1[k] - a2[k];
 *     out_da[r][c][2k] = db[0] e0 + db[2] e1,   out_da[r][c][2k+1] = db[1] e0 + db[3] e1,   db = rast_db[r][c].
 * 0 on background and for an index out of range.  (For uv attributes this is uv_da of the sampler in its order.)
 *
 * ---- the pyramid -----------------------------------------------------------------------------------------------------
 * Level l has Wl = max(Wt >> l, 1) and Hl likewise; levels 0 .. L with L = min(max_mip_level, log2(max(Wt, Ht))), or that
 * logarithm when max_mip_level < 0.  L > 0 needs both sides to be powers of two.  All levels live in ONE buffer of texels
 * of GD_SAMPLE_TEXEL = 4 floats (channels C .. 3 hold 0), so that a tap is one 16-byte load; level l starts at texel
 * offset[l], offset[L + 1] is the total.  Level 0 is the texture.  Texel (x, y) of level l + 1, with parents in level l
 *     both sides of l above 1:   a = (2x, 2y), b = (2x+1, 2y), c = (2x, 2y+1), d = (2x+1, 2y+1):  ((a + b) + (c + d)) 0.25
 *     Wl == 1:                   a = (0, 2y), b = (0, 2y+1):   (a + b) 0.5
 *     Hl == 1:                   a = (2x, 0), b = (2x+1, 0):   (a + b) 0.5
 *
 * ---- sampling --------------------------------------------------------------------------------------------------------
 * uv [N][2], uv_da [N][4] = (du/dX, du/dY, dv/dX, dv/dY), out [N][C].  Texel centres of level l are at (i + 0.5) / Wl.
 * A pixel whose u or v is not finite writes zeros (and has no gradient).
 * index(i, n): i is first clamped to [-2^30, 2^30] as a float and converted; wrap: ((i mod n) + n) mod n; clamp:
 *              min(max(i, 0), n - 1).
 * nearest:     ix = index(floor(u float(Wt)), Wt), iy = index(floor(v float(Ht)), Ht);  out = level0[iy][ix].
 * bilinear(l): xs = u float(Wl), x0 = floor(xs - 0.5), fx = (xs - x0) - 0.5;  ys, y0, fy likewise with v and Hl
 *              (x = u Wl - 0.5, x0 = floor(x), fx = x - x0 in an order that loses nothing for a power-of-two side: xs is
 *              then exact and so are both differences; fx may leave [0, 1) by a rounding, which the blend continues);
 *              columns index(x0), index(x0 + 1), rows index(y0), index(y0 + 1);  t00 = [y0][x0], t10 = [y0][x1],
 *              t01 = [y1][x0], t11 = [y1][x1];
 *              p = t00 + fx (t10 - t00),  q = t01 + fx (t11 - t01),  out = p + fy (q - p).
 * linear:      bilinear(0).
 * level:       sx = uv_da[0] float(Wt), sy = uv_da[1] float(Wt), tx = uv_da[2] float(Ht), ty = uv_da[3] float(Ht);
 *              A = sx sx + tx tx,  B = sy sy + ty ty,  Cc = sx sy + tx ty,  d = A - B;
 *              m = 0.5 (A + B) + sqrt(0.25 (d d) + Cc Cc)         (the squared larger singular value of the Jacobian)
 *              level = min(max(0.5 log2(m), 0), float(L));  m <= 0 or m not finite: level = 0.
 *              (log2 is the device's log2f: the one operation here that is not correctly rounded.)
 * linear-mipmap-nearest:  bilinear(int(floor(level + 0.5))).
 * linear-mipmap-linear:   l0 = int(floor(level)), f = level - float(l0), l1 = min(l0 + 1, L);  c0 = bilinear(l0);
 *              f == 0: out = c0 and l1 is not read;  else c1 = bilinear(l1), out = c0 + f (c1 - c0).
 *
 * ---- gradient to the texture -----------------------------------------------------------------------------------------
 * An item is (pixel n, tap j), item index n T + j: T = 1 (nearest), 4 (linear, linear-mipmap-nearest: taps 00, 10, 01, 11)
 * or 8 (linear-mipmap-linear: the four of l0, then the four of l1).  Its key is the tap's texel index in the pyramid
 * buffer, offset[l] + row Wl + column; its value is weight_j dout[n][k], k < C, the weight rounded before the product:
 *     gx = 1 - fx, gy = 1 - fy;  w00 = gx gy, w10 = fx gy, w01 = gx fy, w11 = fx fy;
 *     linear-mipmap-linear with f != 0: (1 - f) w_j for l0 and f w_j for l1;  nearest: the value is dout[n][k] itself.
 * Items of a pixel with a non-finite u or v, and the l1 items where f == 0, get the key offset[L + 1], which sorts last.
 *   1. gd_sample_texture_items writes keys int64 [N T] and values float [N T][C].
 *   2. The caller sorts the keys STABLY and passes the sorted keys with the permutation (order[i] = the item at sorted
 *      position i).
 *   3. gd_sample_texture_reduce: the first position of each key below offset[L + 1] adds its run in sorted order, i.e. in
 *      ascending item index, starting from +0.0f, and stores the sum to gpyr (the pyramid's gradient, texels of 4 floats;
 *      texels without an item are not written: the caller zeroes gpyr).
 *   4. gd_sample_texture_fold: for l = L - 1 down to 0, g_l[y][x] = g_l[y][x] + w g_{l+1}[y >> 1][x >> 1] with w = 0.25
 *      where both sides of level l exceed 1, else 0.5 (each fine texel reads its single parent; the product is rounded,
 *      then the sum); then dtex[y][x][k] = dtex[y][x][k] + g_0[y][x][k] wherever g_0[y][x][k] != 0: one add per texel,
 *      and a texel nothing reaches keeps its bits.
 *
 * Return 0 on success, negative on error (gd_mesh_last_error()); arguments are validated before the device is touched.
 */
#ifndef GD_SAMPLE_H_INCLUDED
#define GD_SAMPLE_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_SAMPLE_MAX_SIDE 16384
#define GD_SAMPLE_MAX_LEVELS 15      /* levels 0 .. 14 of a side of 16384 */
#define GD_SAMPLE_MAX_CHANNELS 4
#define GD_SAMPLE_TEXEL 4            /* floats per texel of the pyramid buffer */

#define GD_SAMPLE_NEAREST 0
#define GD_SAMPLE_LINEAR 1
#define GD_SAMPLE_LINEAR_MIPMAP_NEAREST 2
#define GD_SAMPLE_LINEAR_MIPMAP_LINEAR 3

#define GD_SAMPLE_WRAP 0
#define GD_SAMPLE_CLAMP 1

/* passed by value; filled by gd_sample_pyramid_layout */
typedef struct gd_sample_pyramid {
    int32_t levels;                              /* L + 1 */
    int32_t width[GD_SAMPLE_MAX_LEVELS];
    int32_t height[GD_SAMPLE_MAX_LEVELS];
    int32_t offset[GD_SAMPLE_MAX_LEVELS + 1];    /* in texels; offset[levels] is the total (below 2^29) */
} gd_sample_pyramid;

/* Host only.  max_mip_level < 0: down to 1 x 1.  More than one level needs power-of-two sides. */
int gd_sample_pyramid_layout(int Ht, int Wt, int max_mip_level, gd_sample_pyramid* out);

/* taps per pixel of a filter mode (1, 4, 4, 8); negative for an unknown mode */
int gd_sample_taps(int filter);

/* rast: float [H][W][4]; pos: float [V][4] (what rast was made from); tri: int32 [F][3]; rast_db: float [H][W][4] out */
int gd_sample_rast_db(void* stream, int V, int F, int H, int W, const float* rast, const float* pos, const int* tri,
                      float* rast_db);

/* attr: float [V][C], 1 <= C <= GD_MESH_MAX_CHANNELS (8); out_da: float [H][W][2C] */
int gd_sample_interpolate_da(void* stream, int V, int F, int C, int H, int W, const float* attr, const float* rast,
                             const float* rast_db, const int* tri, float* out_da);

/* tex: float [Ht][Wt][C] (the sides of layout's level 0), 1 <= C <= 4; pyr: float [offset[levels]][4], every element
 * written */
int gd_sample_build_mips(void* stream, int C, const float* tex, gd_sample_pyramid layout, float* pyr);

/* uv_da may be null for GD_SAMPLE_NEAREST and GD_SAMPLE_LINEAR; 1 <= N, N * taps < 2^31 */
int gd_sample_texture_forward(void* stream, int N, int C, int filter, int boundary, gd_sample_pyramid layout,
                              const float* pyr, const float* uv, const float* uv_da, float* out);

/* keys: int64 [N taps]; vals: float [N taps][C] */
int gd_sample_texture_items(void* stream, int N, int C, int filter, int boundary, gd_sample_pyramid layout,
                            const float* uv, const float* uv_da, const float* dout, int64_t* keys, float* vals);

/* items = N taps; sorted_keys, order: int64 [items]; gpyr: float [offset[levels]][4], zeroed by the caller */
int gd_sample_texture_reduce(void* stream, int64_t items, int C, gd_sample_pyramid layout, const int64_t* sorted_keys,
                             const int64_t* order, const float* vals, float* gpyr);

/* gpyr is folded in place; dtex: float [Ht][Wt][C], added to */
int gd_sample_texture_fold(void* stream, int C, gd_sample_pyramid layout, float* gpyr, float* dtex);

#ifdef __cplusplus
}
#endif
#endif
