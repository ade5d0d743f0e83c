/*
 * gd_mesh.h -- C-ABI of the triangle-mesh render path of the NeTF stage, exported by libgd_raster.so
 * (csrc/raster_mesh.hip).  Plain device pointers, caller's HIP stream, caller-owned scratch, no torch types, no host
 * synchronisation inside any entry, reruns bit-identical.
 *
 *   gd_mesh_rasterize             <- nvdiffrast rasterize     (Garment_Deformer_NeTF/netf/render/mesh_renderer.py:360,
 *   gd_mesh_interpolate_forward   <- nvdiffrast interpolate    :365-368, :398; deformer/core/renderer.py:92-157)
 *   gd_mesh_interpolate_backward     its gradient w.r.t. the attributes
 *   gd_mesh_antialias_weights     <- nvdiffrast antialias     (:363, :378, :404-405): the silhouette analysis, ONCE per
 *   gd_mesh_antialias_apply          (rast, pos), and the blend / its adjoint for every image that shares them
 *
 * Two limits, both those of the reference's live configuration (fix_geo: true, cameras orbiting outside the mesh):
 *   1. no gradient w.r.t. vertex positions in the fixed-geometry entries (nvdiffrast's rast_db and the position
 *      gradient of antialias): those are the entries of gd_mesh_deform.h, defined at the end of this comment;
 *   2. no near-plane clipping: a triangle with a vertex at w <= 0 is DROPPED, not clipped.
 *
 * ---- rasterize: the definition (fp32, one rounding per operation in the stated order; edges in int64) --------------
 * Per vertex:   rw = 1/w;  xn = x rw, yn = y rw, zn = z rw;
 *               X = (int) rintf((xn 0.5 + 0.5) float(256 W)),  Y likewise with H    (8 sub-pixel bits, half to even).
 *               The vertex is unusable if w <= 0, any of rw xn yn zn is not finite, or |X| or |Y| > 2^24;
 *               a triangle with an unusable vertex (or an index outside [0, V)) is dropped.
 * Per triangle: pixel (r, c) has centre Px = 256 c + 128, Py = 256 r + 128 (row 0 is y_ndc = -1, OpenGL's convention);
 *               E0 = (X2-X1)(Py-Y1) - (Y2-Y1)(Px-X1), E1 and E2 cyclically (Ei is opposite vertex i); A = E0+E1+E2.
 *               A == 0: dropped.  A < 0: all three edge functions (and edge vectors) are negated; no culling.
 *               Covered iff for every i: Ei > 0, or Ei == 0 and the edge vector (dX, dY) has dY > 0 or
 *               (dY == 0 and dX < 0): a shared edge belongs to exactly one of its two triangles.
 * Per covered pixel: bi = float(Ei) / float(A);  zw = (b0 zn0 + b1 zn1) + b2 zn2, -0 -> +0; rejected unless
 *               -1 <= zw <= 1;  pi = bi rwi;  s = (p0 + p1) + p2;  u = p0 / s,  v = p1 / s.
 * Visibility:   smallest zw wins; equal bits: lowest triangle index.
 * rast[r][c] = (u, v, zw, float(index + 1)); all four 0 where nothing is covered.  F < 2^24.
 *
 * ---- gradients to vertex positions: the definition (entries: gd_mesh_deform.h) ---------------------------------------
 * The forward stays the one above, with snapped vertices and integer edges.  The gradients are those of the same
 * functions with the snapping removed and every discrete decision of the forward held fixed: the triangle id per pixel,
 * the chosen triangle, edge and side of each antialias pair, and its t <= 1 and t > 0.5 branches (nvdiffrast does the
 * same).  pos is the fp32 clip position [V][4]; z never receives a gradient.
 * rasterize:    pixel (r, c) won by triangle t: fx = (2c + 1)/W - 1, fy = (2r + 1)/H - 1; for its corners
 *               q_i = (x_i - fx w_i, y_i - fy w_i);  a0 = q1 x q2, a1 = q2 x q0, a2 = q0 x q1 (2-D cross products);
 *               u = a0 / (a0 + a1 + a2), v = a1 / (a0 + a1 + a2).  dpos is the exact derivative of this (u, v) in
 *               x, y, w of the three corners, contracted with drast[..., 0:2]; drast[..., 2:4] (z/w, id) is ignored.
 * interpolate:  drast.u = sum_k dout_k (a0_k - a2_k), drast.v = sum_k dout_k (a1_k - a2_k) with a_i = attr[tri[id][i]];
 *               channels 2 and 3 and background pixels are 0.
 * antialias:    every pair whose analysis (below, at gd_mesh_antialias_weights) finds an edge (a, b) of the chosen
 *               triangle with t <= 1 has the weight w = t - 0.5 onto O (t > 0.5) or w = 0.5 - t onto I (t <= 0.5), and
 *               dL/dw = sum_k dout[O]_k (in[I]_k - in[O]_k) or sum_k dout[I]_k (in[O]_k - in[I]_k) respectively.
 *               t = |x* - centre_I| with x* the formula below on the unsnapped sx = (x/w 0.5 + 0.5) W,
 *               sy = (y/w 0.5 + 0.5) H.  dL/dw is chained through +-1, sign(x* - centre_I) and x* to x, y, w of the
 *               vertices a and b.  Each pair counts once, from pixel I's side; pairs without such an edge contribute 0.
 *
 * Return 0 on success, negative on error (gd_mesh_last_error()).
 */
#ifndef GD_MESH_H_INCLUDED
#define GD_MESH_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_MESH_MAX_CHANNELS 8       /* interpolate: C <= 8 */
#define GD_MESH_LARGE_BOX 256        /* pixel bounding boxes above this go to the one-wave-per-triangle kernel */

/* bytes of device scratch gd_mesh_rasterize needs */
size_t gd_mesh_rasterize_scratch_bytes(int F, int H, int W);

/* pos: float [V][4] clip space; tri: int32 [F][3]; rast: float [H][W][4] out. */
int gd_mesh_rasterize(void* stream, int V, int F, int H, int W, const float* pos, const int* tri, float* rast,
                      void* scratch);

/* out[r][c][k] = (u a0[k] + v a1[k]) + ((1 - u) - v) a2[k] with a_i = attr[tri[id][i]]; 0 on background.
 * attr: float [V][C]; out: float [H][W][C]; 1 <= C <= GD_MESH_MAX_CHANNELS. */
int gd_mesh_interpolate_forward(void* stream, int V, int F, int C, int H, int W, const float* attr, const float* rast,
                                const int* tri, float* out);

/* bytes of device scratch gd_mesh_interpolate_backward needs: the [F][3][C] corner-gradient slab */
size_t gd_mesh_interpolate_backward_scratch_bytes(int F, int C);

/* dattr[V][C] from dout[H][W][C], without atomics: one wave per triangle walks the triangle's pixel bounding box
 * (recomputed from pos: the pos the rast came from) in lane-strided order, keeps the pixels whose rast id is this
 * triangle, reduces in a fixed tree and stores three corner gradients; one thread per (vertex, channel) then sums the
 * vertex's corners in the order of corner_idx.  corner_ptr: int32 [V+1], corner_idx: int32 [3F] (corner = 3 t + i,
 * ascending per vertex).  Every element of dattr is written. */
int gd_mesh_interpolate_backward(void* stream, int V, int F, int C, int H, int W, const float* pos, const int* tri,
                                 const float* rast, const float* dout, const int* corner_ptr, const int* corner_idx,
                                 float* dattr, void* scratch);

/* wts[r][c][k], k = (left, right, row - 1, row + 1): the weight pixel (r, c) receives from that neighbour.
 * opp: int32 [F][3]: for edge i of triangle t (opposite vertex i) the vertex of the one other triangle on that edge
 * that is not on the edge, -1 if the edge has != 2 triangles.
 * Edge (a, b) of t with own opposite vertex c and d = opp is a SILHOUETTE iff d < 0, or d is unusable (w_d <= 0, see
 * above), or the int64 side values (Xb-Xa)(Yq-Ya) - (Yb-Ya)(Xq-Xa) of q = c and q = d do not have opposite signs.
 * Pair (p, n) of horizontally / vertically adjacent pixels with different ids: the chosen triangle is the
 * non-background one, else the one with smaller zw, else the lower id; its pixel is I, the other O.  Over the chosen
 * triangle's silhouette edges in order 0, 1, 2 take the first that straddles the line through the two centres
 * (horizontal pair: (Ya <= Py) != (Yb <= Py)) with t <= 1, where, with sx = float(X) / 256 etc. and py = r + 0.5:
 *   x* = sxa + (sxb - sxa) ((py - sya) / (syb - sya)),  t = |x* - cx_I|      (vertical pairs swap x and y).
 * t > 0.5: O receives t - 0.5 of I's value; otherwise I receives 0.5 - t of O's.  No such edge: no weight. */
int gd_mesh_antialias_weights(void* stream, int V, int F, int H, int W, const float* rast, const float* pos,
                              const int* tri, const int* opp, float* wts);

/* adjoint == 0: out[p] = in[p] + sum_k wts[p][k] (in[n_k] - in[p]), k in order, terms with a zero weight skipped.
 * adjoint != 0: out[p] = in[p] (1 - sum_k wts[p][k]) + sum_k wts[n_k][opposite(k)] in[n_k]   (din from dout).
 * in / out: float [H][W][C], any C >= 1; must not alias. */
int gd_mesh_antialias_apply(void* stream, int C, int H, int W, const float* in, const float* wts, float* out,
                            int adjoint);

const char* gd_mesh_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
