/*
 * gd_mesh_clean.h -- C-ABI and DEFINITIONS of mesh cleaning: weld close vertices, drop null and duplicate faces, drop small
 * connected components, repair non-manifold edges and vertices (the place of kiui's clean_mesh, a chain of MeshLab
 * filters, which Garment_Deformer_NeTF/netf/render/mesh_renderer.py:114-121 and :330 call on the mesh they load),
 * exported by libgd_raster.so (csrc/raster_clean.hip).  garmentdreamer_amd/mesh_clean.py drives the entries;
 * tests/clean_reference.py states them sequentially in numpy.  The definitions are this project's own: agreement with
 * MeshLab is not sought and unverified.
 *
 * Same contract as gd_atlas.h: plain device pointers, the caller's HIP stream, no host synchronisation inside any entry,
 * every output element written, no float atomics, reruns bit-identical.  Every entry validates its arguments before any
 * device work: a null pointer or a size outside its range returns -1 with a message in gd_mesh_last_error().  Return 0 on
 * success, -1 on a bad call, -2 on a HIP error.  1 <= V, 1 <= F < 2^29.  Built with -ffp-contract=off: fl(x) below is one
 * IEEE fp32 rounding, and every fp32 operation is rounded on its own.
 *
 * stats: int32 [GD_MESH_CLEAN_STATS], zeroed by the caller once and only ever added to (integer atomics, one per workgroup
 * and quantity) by the entries that name it; the slots are the GD_MESH_CLEAN_STAT_* below.
 *
 * ---- 0. ARGUMENTS ----------------------------------------------------------------------------------------------------
 * check: used[v] = 1 iff some face names v.  An index outside [0, V) raises STAT_INDEX; a referenced vertex with a
 * position that is not finite raises STAT_NONFINITE; the caller raises before anything else runs.  STAT_REFERENCED
 * receives the number of referenced vertices.
 *
 * ---- 1. BOX ----------------------------------------------------------------------------------------------------------
 * box = (min x, min y, min z, max x, max y, max z) over the referenced vertices, exact, by integer atomics on the keys of
 * gd_atlas.h section 3, combined per workgroup in LDS first.  D = sqrt((dx dx + dy dy) + dz dz) in float64 with
 * d = (double) max - (double) min, computed by the host.  D is measured ONCE, on the input, and both percentages refer to
 * it.  (MeshLab measures the box again before every filter; after fragments have been removed its percentages refer to a
 * smaller box than ours.)
 *
 * ---- 2. MERGE --------------------------------------------------------------------------------------------------------
 * r = (float) (D merge_pct / 100), r2 = fl(r r).  With d = fl(a - b) per component, vertices a and b are CLOSE iff
 *     fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)) <= r2                                    (inclusive).
 * Sequentially: the referenced vertices in ascending index; an unassigned v becomes a CENTRE and every unassigned vertex
 * close to v is assigned to v.  Equivalently: the centres are the lexicographically first maximal independent set of the
 * closeness graph and every other vertex goes to its lowest-index close centre.  target[v] = that centre (v itself for a
 * centre, -1 for a vertex no face names).  A centre keeps its position; no coordinate is the result of arithmetic.
 * GRID (gd_remesh_grid of gd_mesh_remesh.h): origin = the box minimum, cell >= max(r, 2^-60) (1 + 2^-20), doubled until the
 * grid has at most 2^21 cells.  The cell of x along an axis is (int) min(max(floorf(fl(fl(x - origin) / cell)), 0), dim - 1),
 * a monotone function of x.  Closeness implies |a - b| <= r (1 + 2^-24) + 2^-74 per axis, so every vertex close to v lies
 * in the cells between that of nextafterf(fl(x - cell), -inf) and that of nextafterf(fl(x + cell), +inf) on each axis:
 * three per axis as a rule, 27 cells.  grid_bin with scatter = 0 counts the referenced vertices per cell; the caller scans;
 * scatter = 1 writes items (the order within a cell is not used by anything below).
 * ROUNDS on state[v] in {0 undecided, 1 centre, 2 merged}, Jacobi (a round reads state_in and writes state_out): an
 * undecided v looks at the close vertices with a lower index: if any is a centre, v is merged; if all are merged, or there
 * are none, v is a centre; otherwise v stays undecided.  undecided[k] = the number of vertices round k left undecided.  A
 * round decides at least the lowest undecided vertex and never revises a decision, so V rounds suffice and the fixed point
 * is the sequential result.  merge_rounds of one call runs `rounds` (even) rounds state_a -> state_b -> state_a; rounds
 * after the fixed point change nothing.
 *
 * ---- 3. NULL FACES ---------------------------------------------------------------------------------------------------
 * relabel: tri_out[f][i] = target[tri[f][i]] (tri itself when target is null).  A face is NULL, alive[f] = 0, iff it names
 * a vertex twice, or its normal n of gd_atlas.h section 1 is (0, 0, 0) or has a component that is not finite.
 * akey[f] = fl(fl(fl(nx nx) + fl(ny ny)) + fl(nz nz)), the AREA KEY of step 6 (0 for a null face).
 *
 * ---- 4. EDGE TABLE AND DUPLICATE FACES -------------------------------------------------------------------------------
 * edge_keys: hkeys[3f + i] = (min(p, q) << 32) | max(p, q) with (p, q) the two vertices of f other than corner i, for a face
 * with alive[f] != 0 that names three distinct vertices; INT64_MAX otherwise.  The caller sorts them stably with their
 * half-edge indices.  edge_table: she[j] = the half-edge at sorted position j (-1 for INT64_MAX), pos[h] = the sorted
 * position of half-edge h.  A RUN is a maximal range of equal keys: the half-edges of one edge, in ascending face order.
 * The table is built once and stays; every later step reads a liveness array next to it.
 * Face f is a DUPLICATE iff a face g < f in the run of f's lowest-key edge names the same opposite vertex, that is the
 * same unordered triple, whatever the orientation: the lowest face index of each triple stays.
 *
 * ---- 5. COMPONENTS ---------------------------------------------------------------------------------------------------
 * Live faces f and g are JOINED iff they share an edge (all faces of a non-manifold edge are joined; faces that share only
 * a vertex are not).  label[f] = the lowest face index of f's component, -1 for a face that is not alive.  face_sweeps
 * runs `sweeps` sweeps of hooking plus pointer jumping (gd_atlas.h section 2, its proof and its cap GD_ATLAS_MAX_SWEEPS)
 * on parent [F]: one lane per sorted position hooks its face to the previous LIVE face of its run.  changed[s] = 1 iff
 * sweep s hooked anything; the labels are final when a sweep changed nothing.
 * component_stats: per label, the face count and the exact fp32 bounding box over the corners of its faces, by integer
 * atomics combined per workgroup in LDS.  component_filter: with e = fl(max - min) per axis, a component is REMOVED iff
 *     (min_faces > 0 and count < min_faces)  or  (t2 > 0 and fl(fl(fl(ex ex) + fl(ey ey)) + fl(ez ez)) < t2),
 * t2 = fl(t t), t = (float) (D min_diameter_pct / 100), t2 = 0 for a percentage <= 0.
 *
 * ---- 6. NON-MANIFOLD EDGES -------------------------------------------------------------------------------------------
 * Rounds on the fixed table, Jacobi on live: every edge with more than two live faces nominates its live face of smallest
 * area key, the highest face index among equal keys; all nominated faces die (a plain store of 0 into live_out, which
 * starts as a copy of live_in).  over[k] = the number of edges round k found with more than two live faces.  Rounds repeat
 * until that is 0: at most the highest edge valence - 2 rounds.
 *
 * ---- 7. NON-MANIFOLD VERTICES ----------------------------------------------------------------------------------------
 * Corners (f, i) and (g, j) of one vertex v belong to one FAN iff f and g are joined by a chain of live faces, each sharing
 * with the next an edge incident to v.  corner_sweeps finds the fans by the same hooking over the 3F corners: one lane per
 * sorted position hooks, for each of the two vertices of its edge, its face's corner of that vertex to the corner of the
 * previous live face of the run.  The fan that holds the lowest live corner index 3f + i of v keeps v.  Every other fan
 * receives a COPY of v at the same position; the copies are appended after the last original vertex in the order of
 * (v, lowest corner of the fan): split_key = (v << 32) | corner for the root corner of such a fan, INT64_MAX elsewhere,
 * sorted by the caller; fan_ranks scatters the rank of each root.
 *
 * ---- 8. OUTPUT -------------------------------------------------------------------------------------------------------
 * emit: the live faces in ascending input order (face_map [F'] -> input face); the vertices they name in ascending input
 * order (V0 rows), then the S copies.  vertex_map[v] = the output row of target[v], -1 if nothing names it any more; for a
 * split vertex the row of the fan that kept it.  Face orientation is not repaired.
 */
#ifndef GD_MESH_CLEAN_H_INCLUDED
#define GD_MESH_CLEAN_H_INCLUDED

#include "gd_mesh_remesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GD_MESH_CLEAN_STATS 16
#define GD_MESH_CLEAN_STAT_INDEX 0
#define GD_MESH_CLEAN_STAT_NONFINITE 1
#define GD_MESH_CLEAN_STAT_REFERENCED 2
#define GD_MESH_CLEAN_STAT_MERGED 3
#define GD_MESH_CLEAN_STAT_NULL 4
#define GD_MESH_CLEAN_STAT_DUPLICATE 5
#define GD_MESH_CLEAN_STAT_COMPONENTS 6
#define GD_MESH_CLEAN_STAT_COMPONENTS_REMOVED 7
#define GD_MESH_CLEAN_STAT_COMPONENT_FACES 8
#define GD_MESH_CLEAN_STAT_SPLIT 9
#define GD_MESH_CLEAN_MAX_ROUNDS 16   /* rounds or sweeps of one call */
#define GD_MESH_CLEAN_MAX_CELLS (1 << 21)

/* used: int32 [V] out; box: float [6] out; box_keys: uint32 [6] scratch. */
int gd_mesh_clean_check(void* stream, int V, int F, const float* verts, const int32_t* tri, int32_t* used, float* box,
                        uint32_t* box_keys, int32_t* stats);

/* scatter == 0: count [cells], zeroed by the caller, receives the referenced vertices per cell.  scatter != 0: start
 * [cells + 1] is its exclusive scan, count is zeroed again by the caller, items: int32 [V] out (-1 past the referenced). */
int gd_mesh_clean_grid_bin(void* stream, const gd_remesh_grid* grid, int V, const float* verts, const int32_t* used,
                           int scatter, int32_t* count, const int32_t* start, int32_t* items);

/* state_a: int32 [V] in/out (0 at the start); state_b: int32 [V] scratch; undecided: int32 [rounds] out. */
int gd_mesh_clean_merge_rounds(void* stream, const gd_remesh_grid* grid, int V, const float* verts, const int32_t* used,
                               const int32_t* start, const int32_t* items, float r2, int rounds, int32_t* state_a,
                               int32_t* state_b, int32_t* undecided);

/* merge == 0: target[v] = v for a referenced vertex, and grid, start, items and state may be null.  target: int32 [V] out. */
int gd_mesh_clean_merge_target(void* stream, const gd_remesh_grid* grid, int V, const float* verts, const int32_t* used,
                               const int32_t* start, const int32_t* items, float r2, int merge, const int32_t* state,
                               int32_t* target, int32_t* stats);

/* target: int32 [V] or null; tri_out: int32 [F][3] out; alive: int32 [F] out; akey: float [F] out. */
int gd_mesh_clean_relabel(void* stream, int V, int F, const float* verts, const int32_t* tri, const int32_t* target,
                          int32_t* tri_out, int32_t* alive, float* akey, int32_t* stats);

/* hkeys: int64 [3F] out. */
int gd_mesh_clean_edge_keys(void* stream, int V, int F, const int32_t* tri, const int32_t* alive, int64_t* hkeys);

/* n = 3F; skeys, order: int64 [n], the stable sort of hkeys; she, pos: int32 [n] out. */
int gd_mesh_clean_edge_table(void* stream, int n, const int64_t* skeys, const int64_t* order, int32_t* she, int32_t* pos);

/* alive_out: int32 [F] out, not alive_in. */
int gd_mesh_clean_duplicates(void* stream, int F, const int32_t* tri, const int32_t* alive_in, const int64_t* skeys,
                             const int32_t* she, const int32_t* pos, int32_t* alive_out, int32_t* stats);

/* init != 0: parent[f] = f first.  parent: int32 [F] in/out; changed: int32 [sweeps] out. */
int gd_mesh_clean_face_sweeps(void* stream, int F, const int64_t* skeys, const int32_t* she, const int32_t* alive,
                              int sweeps, int init, int32_t* parent, int32_t* changed);

/* ckeys: uint32 [F][6] out (row l: the keys of the box of the component labelled l); ccount: int32 [F] out. */
int gd_mesh_clean_component_stats(void* stream, int V, int F, const float* verts, const int32_t* tri, const int32_t* alive,
                                  const int32_t* parent, uint32_t* ckeys, int32_t* ccount);

/* label, alive_out: int32 [F] out, alive_out not alive_in. */
int gd_mesh_clean_component_filter(void* stream, int F, const int32_t* alive_in, const int32_t* parent,
                                   const uint32_t* ckeys, const int32_t* ccount, int min_faces, float t2, int32_t* label,
                                   int32_t* alive_out, int32_t* stats);

/* live_a: int32 [F] in/out; live_b: int32 [F] scratch; rounds even; over: int32 [rounds] out. */
int gd_mesh_clean_edge_rounds(void* stream, int F, const int64_t* skeys, const int32_t* she, const float* akey, int rounds,
                              int32_t* live_a, int32_t* live_b, int32_t* over);

/* parent: int32 [3F] in/out; changed: int32 [sweeps] out. */
int gd_mesh_clean_corner_sweeps(void* stream, int F, const int32_t* tri, const int64_t* skeys, const int32_t* she,
                                const int32_t* alive, int sweeps, int init, int32_t* parent, int32_t* changed);

/* parent: int32 [3F] or null (then nothing is split and vmin and split_key may be null).  vmin: int32 [V] scratch;
 * used: int32 [V] out; split_key: int64 [3F] out. */
int gd_mesh_clean_fan_roots(void* stream, int V, int F, const int32_t* tri, const int32_t* alive, const int32_t* parent,
                            int32_t* vmin, int32_t* used, int64_t* split_key, int32_t* stats);

/* n = 3F; sorted_keys: int64 [n], split_key sorted, its first S below INT64_MAX; crank: int32 [n] out. */
int gd_mesh_clean_fan_ranks(void* stream, int n, int S, const int64_t* sorted_keys, int32_t* crank);

/* The faces alone, for a single pass: fscan: int32 [F+1], the exclusive scan of alive, Fout = fscan[F] >= 1 as the caller
 * read it.  tri_out: int32 [Fout][3] out, the rows of tri with alive != 0 in their order; face_map: int32 [Fout] out. */
int gd_mesh_clean_compact_faces(void* stream, int F, int Fout, const int32_t* tri, const int32_t* alive,
                                const int32_t* fscan, int32_t* tri_out, int32_t* face_map);

/* fscan: int32 [F+1] and vscan: int32 [V+1], the exclusive scans of alive and used, with Fout = fscan[F] >= 1 and
 * V0 = vscan[V] as the caller read them.  target: int32 [V] or null (the identity on used vertices).  parent, crank and
 * sorted_keys are null iff S == 0.  verts_out: float [V0 + S][3]; tri_out: int32 [Fout][3]; face_map: int32 [Fout];
 * vertex_map: int32 [V]: all out. */
int gd_mesh_clean_emit(void* stream, int V, int F, int Fout, int V0, int S, const float* verts, const int32_t* tri,
                       const int32_t* alive, const int32_t* fscan, const int32_t* used, const int32_t* vscan,
                       const int32_t* target, const int32_t* parent, const int32_t* crank, const int64_t* sorted_keys,
                       float* verts_out, int32_t* tri_out, int32_t* face_map, int32_t* vertex_map);

#ifdef __cplusplus
}
#endif
#endif
