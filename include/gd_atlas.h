/*
 * gd_atlas.h -- C-ABI and DEFINITIONS of the chart-based UV atlas of the textured-mesh export (the place of xatlas in
 * the reference's mesh.auto_uv, Garment_Deformer_NeTF/netf/render/mesh_renderer.py:267), exported by libgd_raster.so
 * (csrc/raster_atlas.hip).  A different algorithm from xatlas, and no agreement with it is sought: a normal-bucketed
 * orthographic unwrap.  garmentdreamer_amd/texture_atlas.py drives the entries; tests/atlas_reference.py states them
 * in numpy.
 *
 * Same contract as gd_mesh.h: plain device pointers, caller's HIP stream, no host synchronisation inside any entry,
 * every output element written, no float atomics, reruns bit-identical.  Every entry validates its arguments before any
 * device work: a null pointer or a size outside its range returns -1 with a message in gd_mesh_last_error().
 * Return 0 on success, -1 on a bad call, -2 on a HIP error.  1 <= V, 1 <= F < 2^29, 1 <= E <= 3F, 1 <= C <= F,
 * 1 <= resolution <= GD_ATLAS_MAX_RESOLUTION, 0 <= gutter <= GD_ATLAS_MAX_GUTTER, 0 < scale < inf.
 *
 * ---- 1. FACE CLASS (fp32, one rounding per operation, no contraction) ------------------------------------------------
 * With p_i = verts[tri[f][i]]:  u = p1 - p0,  w = p2 - p0  (per component);
 *     n = (u.y w.z - u.z w.y,  u.z w.x - u.x w.z,  u.x w.y - u.y w.x)      each product rounded, then the difference.
 * k = argmax_k |n_k|, the lowest k among equals;  class = 2k + (n_k < 0).
 * n = (0, 0, 0), a component of n that is not finite, or a vertex index outside [0, V): class 6 = GD_ATLAS_DEGENERATE.
 * A degenerate face takes part in no chart, has face_chart = -1 and receives the single point (0, 0) as its UV.
 * PROJECTED COORDINATES of a class: with k = class / 2, (a, b) = (p[(k+1) % 3], p[(k+2) % 3]) for an even class and
 * (p[(k+2) % 3], p[(k+1) % 3]) for an odd one: the face's area in (a, b) is |n_k| / 2 > 0 for both signs.  a and b
 * are components of the input, not results of arithmetic.
 *
 * ---- 2. CHARTS -------------------------------------------------------------------------------------------------------
 * layer: int32 [F] (0 at the start, raised by the peeling of step 6); single: int32 [F], nonzero = a face that is a
 * chart of its own.  Faces f and g are JOINED iff they are the two faces of an interior edge (eh[e] = (3f + i, 3g + j),
 * both >= 0: the table of gd_mesh_remesh.h), class[f] == class[g] != 6, layer[f] == layer[g], and neither is single.
 * label[f] = the lowest face index of f's connected component under that relation (a degenerate or single face: f).
 * gd_atlas_hook + gd_atlas_jump are one SWEEP of hooking with pointer jumping on parent: int32 [F], parent[f] = f at
 * the start.  hook: per joined pair, the roots r_f, r_g found by following parent; if they differ, atomicMin(parent +
 * max(r_f, r_g), min(r_f, r_g)) and changed[0] = 1.  jump: parent[f] = the root of f.  parent[x] <= x always holds, so
 * following ends, and only members of x's component are ever stored in parent[x].  When a sweep leaves changed[0] == 0
 * every joined pair has one root, so each component has one root, its lowest index: parent == label, whatever the
 * schedule was.  A sweep removes every root that is not the lowest among the roots it is joined to, and the jump makes
 * every tree a star again, so the sweep count does not follow the mesh's diameter (a strip of 4096 faces, a path: 3
 * sweeps, the last of which finds nothing to do); the caller stops with an error after GD_ATLAS_MAX_SWEEPS.
 * gd_atlas_roots: is_root[f] = (parent[f] == f and class[f] != 6).  With scan = the exclusive scan of is_root
 * (gd_mesh_remesh_scan), the chart of a non-degenerate face is scan[label[f]]: charts are numbered by ascending label,
 * C = scan[F].
 *
 * ---- 3. BOUNDS -------------------------------------------------------------------------------------------------------
 * bounds[c] = (a_min, b_min, a_max, b_max) over the 3 corners of every face of chart c, exact: the minimum and maximum
 * are taken by integer atomics on key(x) = bits(x) ^ (bits(x) >> 31 ? 0xFFFFFFFF : 0x80000000), which orders finite
 * floats as the reals are ordered (and -0 below +0); a workgroup first combines its faces in an LDS table and sends one
 * atomic per (chart, quantity) it saw to memory.  count[c] = the number of faces of chart c.
 *
 * ---- 4. PACKING (host, integers; tests/atlas_reference.py and texture_atlas.py hold the same lines) -------------------
 * For a scale s (a float32, texels per unit length) chart c has the inner size, in float32,
 *     m_a = rintf(((a_max - a_min) * s) * 256),   wi = max(ceil(m_a / 256), 1) = max((m_a + 255) div 256, 1),
 * hi likewise from b, and the rectangle (w, h) = (wi + 2 gutter, hi + 2 gutter).  SHELVES: charts sorted by h descending,
 * then w descending, then c ascending; a cursor (x, y) = (0, 0) and a shelf height 0; for each chart: w > resolution
 * fails; if x + w > resolution: y += shelf height, x = 0, and the shelf is new; a new shelf takes this chart's h as its
 * height; y + h > resolution fails; the chart's offset is (ox, oy) = (x, y); x += w.
 * SCALE: fits(0) must hold, else the resolution is too small for the gutters of the charts (ValueError).  With d = the
 * largest a- or b-extent of any chart in float64, hi = (resolution - 2 gutter) / d in float64: if fits(float32(hi)),
 * s = float32(hi); else lo = 0 and GD_ATLAS_BISECTION_STEPS times: mid = float32((lo + hi) / 2); fits(mid) ? lo = mid :
 * hi = mid; s = lo, and s == 0 is the same ValueError.
 *
 * ---- 5. CORNERS ------------------------------------------------------------------------------------------------------
 * In units of 1/256 texel, for corner i of face f of chart c, fp32 in this order:
 *     X = 256 (ox + gutter) + (int) rintf(((a - a_min) * s) * 256),   Y = 256 (oy + gutter) + (int) rintf(((b - b_min) * s) * 256)
 * (rintf is monotone, so 0 <= X - 256 (ox + gutter) <= m_a: the chart stays inside its rectangle's inner part).
 * key = c 2^32 + vertex index.  A degenerate face: X = Y = 0 and key = C 2^32 for each corner.
 * The rows of vt are the distinct keys in ascending order (one row per (chart, vertex) pair, and one for all degenerate
 * corners); ft[f][i] is the row of its key; vt[row] = (float(X) / float(256 resolution), float(Y) / float(256 resolution)).
 * For a power-of-two resolution the rasterizer's own rintf((vt 2 - 1) 0.5 + 0.5) float(256 W)) is X again.
 *
 * ---- 6. LOST FACES ---------------------------------------------------------------------------------------------------
 * rast is gd_mesh_rasterize's image of the atlas at z = 0, w = 1: texel (r, c) is owned by the lowest face index that
 * covers its centre.  Face f, with its corners (X_i, Y_i) and the coverage rule of gd_mesh.h word for word (centre
 * Px = 256 c + 128, Py = 256 r + 128; int64 edge functions; A == 0 covers nothing; A < 0 negates; top-left rule), is
 * LOST iff some texel of the image whose centre it covers has (int) rast[r][c][3] - 1 != f.  lost[f] = 1 or 0.
 * Then, for a lost face: freeze == 0: layer[f] += 1; freeze != 0: single[f] = 1.
 */
#ifndef GD_ATLAS_H_INCLUDED
#define GD_ATLAS_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_ATLAS_DEGENERATE 6
#define GD_ATLAS_MAX_SWEEPS 64
#define GD_ATLAS_MAX_RESOLUTION 16384
#define GD_ATLAS_MAX_GUTTER 64
#define GD_ATLAS_BISECTION_STEPS 24

/* verts: float [V][3]; tri: int32 [F][3]; cls: int32 [F] out. */
int gd_atlas_face_class(void* stream, int V, int F, const float* verts, const int32_t* tri, int32_t* cls);

/* eh: int32 [E][2]; cls, layer, single: int32 [F]; parent: int32 [F] in/out; changed: int32 [1], set to 1 by a hook. */
int gd_atlas_hook(void* stream, int F, int E, const int32_t* eh, const int32_t* cls, const int32_t* layer,
                  const int32_t* single, int32_t* parent, int32_t* changed);

/* parent: int32 [F] in/out. */
int gd_atlas_jump(void* stream, int F, int32_t* parent);

/* is_root: int32 [F] out. */
int gd_atlas_roots(void* stream, int F, const int32_t* cls, const int32_t* parent, int32_t* is_root);

/* scan: int32 [F+1], the exclusive scan of is_root; C = scan[F] as the caller read it.  face_chart: int32 [F] out;
 * keys: uint32 [C][4] scratch; bounds: float [C][4] out; count: int32 [C] out. */
int gd_atlas_bounds(void* stream, int V, int F, int C, const float* verts, const int32_t* tri, const int32_t* cls,
                    const int32_t* parent, const int32_t* scan, int32_t* face_chart, uint32_t* keys, float* bounds,
                    int32_t* count);

/* offsets: int32 [C][2] (ox, oy); corner_xy: int32 [F][3][2] out; key: int64 [3F] out. */
int gd_atlas_emit(void* stream, int V, int F, int C, int resolution, int gutter, float scale, const float* verts,
                  const int32_t* tri, const int32_t* cls, const int32_t* face_chart, const float* bounds,
                  const int32_t* offsets, int32_t* corner_xy, int64_t* key);

/* n = 3F corners; row: int64 [n], each in [0, T); vt: float [T][2] out (every row must occur in row); ft: int32 [n] out. */
int gd_atlas_write_vt(void* stream, int n, int T, int resolution, const int64_t* row, const int32_t* corner_xy, float* vt,
                      int32_t* ft);

/* rast: float [H][W][4]; lost: int32 [F] out; layer, single: int32 [F] in/out. */
int gd_atlas_lost_faces(void* stream, int F, int H, int W, const int32_t* corner_xy, const float* rast, int freeze,
                        int32_t* lost, int32_t* layer, int32_t* single);

#ifdef __cplusplus
}
#endif
#endif
