/*
 * gd_mesh_remesh.h -- C-ABI and DEFINITIONS of the isotropic remesher of the mesh deformer's upsample iterations (the place
 * of gpytoolbox.remesh_botsch in Garment_Deformer_NeTF/deformation.py:273-295), exported by libgd_raster.so
 * (csrc/raster_remesh.hip).  One remesh is `iterations` times  split -> collapse rounds -> flip rounds -> relax -> project
 * (garmentdreamer_amd/mesh_remesh.py drives the passes; tests/remesh_reference.py states them sequentially in numpy).
 *
 * Contract: plain device pointers, the caller's HIP stream, caller-owned buffers, no floating-point atomics, reruns
 * bit-identical.  All arithmetic is fp32 in the order written below (built with -ffp-contract=off).  Every entry validates
 * its arguments on the host first: -1 with a message in gd_mesh_last_error() on a bad call, -2 on a HIP error, 0 otherwise.
 * What only the device can see is reported in `flags` (int32 [GD_REMESH_FLAGS], zeroed by the caller): a kernel that meets
 * an index or a position outside the capacity it was given sets a flag and does not write there.  No entry synchronises;
 * the caller reads flags and counts back where it has to size the next buffer.
 *
 * NOTATION.  |p - q|^2 = (dx dx + dy dy) + dz dz with d = p - q per component; dot(p, q) = (p.x q.x + p.y q.y) + p.z q.z;
 * u x w = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x);  N(p0, p1, p2) = (p1 - p0) x (p2 - p0), never
 * normalised in a decision.  h is the target length, hi = 4/3 h, lo = 4/5 h; the caller passes hi^2 and lo^2 as
 * (float)(hi hi) and (float)(lo lo) of the double products.
 *
 * CONNECTIVITY of tri [F][3] over V vertices (int32), rebuilt at the start of every round:
 *   keys         half-edge k = 3 f + i is edge i of face f, between corners i+1 and i+2 (as _mesh_ops.edge_groups), with
 *                the key (min << 32) | max of its two vertices; corner k has the key (vertex << 32) | k.  A vertex index
 *                outside [0, V) sets FLAG_INDEX, a face that lists a vertex twice FLAG_REPEATED.
 *   the caller   sorts the half-edge keys stably (values and order) and the corner keys.
 *   heads        head[j] = the sorted key j differs from key j-1 (head[0] = 1); key j == key j-2 sets FLAG_NONMANIFOLD.
 *   scan         exclusive scan of head; E = its total.  Edge e is the e-th distinct key, so edges are sorted by (lo, hi).
 *   edge tables  ev[e] = (lo, hi); eh[e] = its one or two half-edges in sorted (= ascending k) order, the second -1 for a
 *                boundary edge; fe[k] = e (face -> 3 edges); bnd[v] = 1 for both ends of a boundary edge (bnd zeroed by the
 *                caller); ukeys[e] = the key, rkeys[e] = (hi << 32) | lo, which the caller sorts.
 *   vertex tables  nbr_ptr[v] = (number of ukeys below v << 32) + (number of sorted rkeys below v << 32), by binary search;
 *                the row of v is the low words of its rkeys (neighbours below v, ascending) and then of its ukeys
 *                (neighbours above v, ascending).  vf_ptr[v] = number of sorted corner keys below v << 32, vf_idx = their
 *                low words: the corners of v, ascending.  A vertex no face names has empty rows and bnd = 0.
 *
 * SPLIT.  mark[e] = |p_lo - p_hi|^2 > hi^2.  Marked edge e becomes vertex V + escan[e] (exclusive scan of mark) at
 *   0.5f (p_lo + p_hi) per component.  Face f = (v0, v1, v2) with midpoints m_i on its marked edges i emits 1 + (marked
 *   edges) faces at fscan[f] (exclusive scan of those counts), in this order:
 *     none     (v0, v1, v2)
 *     one      i = the marked edge, a = v_i, b = v_{i+1}, c = v_{i+2}, m = m_i:   (a, b, m), (a, m, c)
 *     two      i = the UNmarked edge, a, b, c as above, mab = m_{i+2}, mca = m_{i+1}:   (a, mab, mca), then the quad
 *              (mab, b, c, mca) cut along the shorter of  d_b = |p_b - 0.5f (p_c + p_a)|^2  and
 *              d_c = |0.5f (p_a + p_b) - p_c|^2:   d_b <= d_c:  (mab, b, mca), (b, c, mca)    else  (mab, b, c), (mab, c, mca)
 *     three    (v0, m2, m1), (v1, m0, m2), (v2, m1, m0), (m0, m1, m2)
 *
 * COLLAPSE ROUND.  Edge e = (lo, hi) is a candidate when |p_lo - p_hi|^2 < lo^2 and a direction "remove a, keep b where b
 *   is" is allowed, tried as (a, b) = (lo, hi) and then (hi, lo); dir[e] = 0, 1 or 2.  A boundary edge whose face has its
 *   third vertex on the boundary too is never a candidate (a face with three boundary vertices stays: no corner or ear of
 *   the surface is eaten, a lone triangle or quad survives any h).  Allowed means, tested in this order:
 *     bnd[a] implies that e is a boundary edge;  not (bnd[a], bnd[b] and e interior);
 *     |nbr(a) & nbr(b)| = 2 for an interior edge, 1 for a boundary edge;
 *     no n in nbr(a), n != b, has |p_n - p_b|^2 > hi^2;
 *     every corner of a (ascending) whose face does not name b has dot(N(old), N(with p_a replaced by p_b)) > 0, the
 *     face's corners in their stored order.
 *   key = (bits of the fp32 squared length << 32) | e, unsigned 64-bit; a candidate takes atomicMin(key) onto lo, hi and
 *   every vertex of nbr(lo) and nbr(hi) (vkey preset to all ones by the caller); a second kernel selects the candidate iff
 *   all of them hold its key, writes remap[a] = b (remap preset to the identity) and counts it in FLAG_SELECTED.  Selected
 *   collapses have disjoint closed neighbourhoods, so their stars share no face and no remap chains.  relabel maps every
 *   corner through remap and marks the faces that keep three distinct vertices; compact_faces keeps those in order.  Dead
 *   faces are removed after each round, which leaves the same faces in the same order as one removal after the last
 *   round; vertices keep their indices until compact_vertices after the last round.
 *
 * FLIP ROUND.  Interior edge e with half-edges k0 < k1 in faces f0, f1: c = the corner of f0 opposite e, p and q its next
 *   two corners, d the corner of f1 opposite e.  A candidate needs f1 to run (d, q, p) (consistent orientation), c != d,
 *   d not in nbr(c), and with cost(v, s) = |deg(v) + s - (bnd[v] ? 4 : 6)|:
 *     after = cost(p,-1) + cost(q,-1) + cost(c,1) + cost(d,1)  <  before = cost(p,0) + cost(q,0) + cost(c,0) + cost(d,0),
 *   and dot(m, n) > 0 for m in {N(c,p,d), N(c,d,q)}, n in {N(c,p,q), N(d,q,p)}.
 *   key = ((after - before + 2^30) << 32) | e; atomicMin onto c, p, q, d; selected iff all four hold it; then
 *   f0 = (c, p, d) and f1 = (c, d, q) in place.  The apply kernel reads only what the candidate kernel stored.
 *
 * RELAX (Jacobi).  A vertex with bnd = 1 or without neighbours keeps its position and has moved = 0.  Otherwise
 *   s = sum of p_j over nbr(v), ascending, from 0;  d = s / (float)deg - p per component;
 *   n = sum over the corners of v, ascending, from 0, of N(face in its stored order);  n = n / max(sqrtf(dot(n, n)), 1e-12);
 *   t = dot(n, d);  out = p + (d - n t) per component;  moved = 1.
 *
 * PROJECT onto the surface the remesh started from (verts0, tri0).  Grid: cell size c >= max(longest edge of the surface,
 *   hi); origin = its bounding box's minimum; dims_a = floor(extent_a / c) + 1; the caller doubles c until the number of
 *   cells is at most GD_REMESH_MAX_CELLS.  cell(x) = (int) clamp(floorf((x - origin) / c), -2, dims + 1) per axis.
 *   A triangle is listed in every cell of the box cell(min corner) .. cell(max corner), clamped to the grid (count -> scan
 *   -> scatter; at most 8 cells, since no edge is longer than c).  A query scans the cells within 1 of cell(p) on every
 *   axis and keeps the smallest |r - p|^2, r = closest(p; a, b, c) below, the lowest triangle index on a tie, so the order
 *   inside a cell does not matter.  best <= c c: out = r; otherwise out = p and FLAG_UNPROJECTED counts it.  If the
 *   closest point of the whole surface lies within c of p, its cell is within 1 of cell(p) on every axis and its triangle
 *   is listed there, so the answer is the exact one.
 *   closest(p; a, b, c), ab = b - a, ac = c - a, in this order (Ericson, Real-Time Collision Detection 5.1.5):
 *     ap = p - a, d1 = dot(ab, ap), d2 = dot(ac, ap):  d1 <= 0 and d2 <= 0 -> a
 *     bp = p - b, d3 = dot(ab, bp), d4 = dot(ac, bp):  d3 >= 0 and d4 <= d3 -> b
 *     vc = d1 d4 - d3 d2:  vc <= 0, d1 >= 0, d3 <= 0 -> a + ab (d1 / (d1 - d3))
 *     cp = p - c, d5 = dot(ab, cp), d6 = dot(ac, cp):  d6 >= 0 and d5 <= d6 -> c
 *     vb = d5 d2 - d1 d6:  vb <= 0, d2 >= 0, d6 <= 0 -> a + ac (d2 / (d2 - d6))
 *     va = d3 d6 - d5 d4:  va <= 0, d4 - d3 >= 0, d5 - d6 >= 0 -> b + (c - b) ((d4 - d3) / ((d4 - d3) + (d5 - d6)))
 *     s = (va + vb) + vc -> (a + ab (vb / s)) + ac (vc / s)
 *   A degenerate triangle whose distance is not a number is never the smallest.
 */
#ifndef GD_MESH_REMESH_H_INCLUDED
#define GD_MESH_REMESH_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    GD_REMESH_FLAG_INDEX = 0,        /* a vertex index outside [0, V) */
    GD_REMESH_FLAG_REPEATED = 1,     /* a face lists a vertex twice */
    GD_REMESH_FLAG_NONMANIFOLD = 2,  /* an edge shared by more than two faces */
    GD_REMESH_FLAG_CAPACITY = 3,     /* a table entry or an output position outside its buffer: nothing was written there */
    GD_REMESH_FLAG_SELECTED = 4,     /* count of the collapses / flips a round applied */
    GD_REMESH_FLAG_UNPROJECTED = 5,  /* count of the queries with no triangle within the cell size */
    GD_REMESH_FLAGS = 8
};
#define GD_REMESH_MAX_CELLS (1 << 21)

/* the connectivity of one round, all device pointers */
typedef struct gd_remesh_mesh {
    int32_t V, F, E;
    const float* verts;     /* [V][3] */
    const int32_t* tri;     /* [F][3] */
    const int32_t* ev;      /* [E][2] */
    const int32_t* eh;      /* [E][2] */
    const int32_t* bnd;     /* [V] */
    const int32_t* nbr_ptr; /* [V+1] */
    const int32_t* nbr_idx; /* [2E] */
    const int32_t* vf_ptr;  /* [V+1] */
    const int32_t* vf_idx;  /* [3F] */
} gd_remesh_mesh;

typedef struct gd_remesh_grid {
    float origin[3];
    float cell;
    int32_t dims[3];
} gd_remesh_grid;

/* out [n+1]: exclusive scan of in [n], the total last; one workgroup, in != out */
int gd_mesh_remesh_scan(void* stream, int n, const int* in, int* out);

int gd_mesh_remesh_keys(void* stream, int V, int F, const int* tri, int64_t* hkeys, int64_t* ckeys, int* flags);
int gd_mesh_remesh_heads(void* stream, int n, const int64_t* sorted_keys, int* head, int* flags);
int gd_mesh_remesh_edge_tables(void* stream, int V, int F, int E, const int64_t* sorted_keys, const int64_t* order,
                               const int* head_scan, int* fe, int* ev, int* eh, int64_t* ukeys, int64_t* rkeys, int* bnd,
                               int* flags);
int gd_mesh_remesh_vertex_tables(void* stream, int V, int F, int E, const int64_t* ukeys, const int64_t* sorted_rkeys,
                                 const int64_t* sorted_ckeys, int* nbr_ptr, int* nbr_idx, int* vf_ptr, int* vf_idx);

int gd_mesh_remesh_split_mark(void* stream, int V, int E, const float* verts, const int* ev, float hi2, int* mark);
int gd_mesh_remesh_split_count(void* stream, int F, int E, const int* fe, const int* mark, int* count);
/* verts_out [Vcap][3]: rows V .. are written (the caller copies rows 0 .. V-1); tri_out [Fcap][3] */
int gd_mesh_remesh_split_apply(void* stream, int V, int F, int E, int Vcap, int Fcap, const float* verts, const int* tri,
                               const int* ev, const int* fe, const int* mark, const int* edge_scan, const int* face_scan,
                               float* verts_out, int* tri_out, int* flags);

int gd_mesh_remesh_collapse_candidates(void* stream, const gd_remesh_mesh* mesh, float lo2, float hi2, int* dir,
                                       uint64_t* ekey, uint64_t* vkey);
int gd_mesh_remesh_collapse_select(void* stream, const gd_remesh_mesh* mesh, const int* dir, const uint64_t* ekey,
                                   const uint64_t* vkey, int* remap, int* flags);
int gd_mesh_remesh_relabel(void* stream, int V, int F, const int* tri, const int* remap, int* tri_out, int* alive, int* flags);
int gd_mesh_remesh_compact_faces(void* stream, int F, int Fcap, const int* tri, const int* alive, const int* alive_scan,
                                 int* tri_out, int* flags);

/* quad [E][4] */
int gd_mesh_remesh_flip_candidates(void* stream, const gd_remesh_mesh* mesh, int* quad, uint64_t* ekey, uint64_t* vkey);
int gd_mesh_remesh_flip_apply(void* stream, int V, int F, int E, const int* eh, const int* quad, const uint64_t* ekey,
                              const uint64_t* vkey, int* tri, int* flags);

int gd_mesh_remesh_relax(void* stream, const gd_remesh_mesh* mesh, float* verts_out, int* moved);

/* scatter = 0: count [cells] += the triangles of each cell; scatter = 1: count (zeroed again) is the cursor, start the scan */
int gd_mesh_remesh_grid_bin(void* stream, const gd_remesh_grid* grid, int V, int F, const float* verts, const int* tri,
                            int scatter, int* count, const int* start, int* items, int capacity, int* flags);
/* moved: null = every point is a query */
int gd_mesh_remesh_project(void* stream, const gd_remesh_grid* grid, int n, const float* points, const int* moved, int V,
                           int F, const float* verts, const int* tri, const int* start, const int* items, int capacity,
                           float* out, int* flags);

int gd_mesh_remesh_used_vertices(void* stream, int V, int F, const int* tri, int* used, int* flags);
int gd_mesh_remesh_compact_vertices(void* stream, int V, int F, int Vcap, const float* verts, const int* tri, const int* used,
                                    const int* used_scan, float* verts_out, int* tri_out, int* flags);

/* len [E] = sqrtf(|p_a - p_b|^2) of edges int64 [E][2] */
int gd_mesh_remesh_edge_lengths(void* stream, int V, int E, const float* verts, const int64_t* edges, float* len);

#ifdef __cplusplus
}
#endif
#endif
