/*
 * gd_mesh_simplify.h -- C-ABI and DEFINITIONS of the deformer's final-mesh post-process (the place of MeshLab's quadric
 * edge-collapse decimation and Taubin smoothing in Garment_Deformer_NeTF/deformer/tools/post_process.py:13-38, called by
 * write_mesh(..., post_process=True), deformer/utils/io.py:18-36), exported by libgd_raster.so (csrc/raster_simplify.hip).
 * garmentdreamer_amd/mesh_simplify.py drives the rounds; tests/simplify_reference.py states them sequentially in numpy.
 *
 * Contract: as include/gd_mesh_remesh.h, whose connectivity (gd_remesh_mesh), flags, scan, relabel, compact_faces and
 * vertex compaction are used unchanged: plain device pointers, the caller's HIP stream, caller-owned buffers, -1 with a
 * message in gd_mesh_last_error() on a bad call, -2 on a HIP error, no entry synchronises.  The only atomics are 64-bit
 * integer atomicMin and an integer counter: no floating-point atomics, reruns bit-identical.  Built with -ffp-contract=off:
 * every operation below is one IEEE add or multiply, in the order written.
 *
 * DECIMATION: half-edge collapses ordered by quadric error, the kept vertex always an endpoint, the boundary kept exactly.
 *
 * QUADRICS, all fp64, from p = (double) of the fp32 positions.  For face f = (v0, v1, v2) in its stored order:
 *     u = p1 - p0, w = p2 - p0;  N = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x), not normalised;
 *     d = -((N.x p0.x + N.y p0.y) + N.z p0.z);
 *     Q_f = (Nx Nx, Nx Ny, Nx Nz, Nx d, Ny Ny, Ny Nz, Ny d, Nz Nz, Nz d, d d)        entries 0 .. 9
 *   (a weight of the squared area: no square root, no division).  Q[v] = the sum of Q_f over the corners of v in the order
 *   of the vf row (ascending), from 0, entry by entry: one lane per vertex, no atomics.  Q is [V][10] and lives through all
 *   rounds: vertices keep their indices until the final compaction.
 *   value(q, p) with the terms  t0 = (q0 x) x, t1 = (q4 y) y, t2 = (q7 z) z, t3 = (q1 x) y, t4 = (q2 x) z, t5 = (q5 y) z,
 *   t6 = q3 x, t7 = q6 y, t8 = q8 z, t9 = q9:
 *     value = ((((t0 + t1) + t2) + 2 ((t3 + t4) + t5)) + 2 ((t6 + t7) + t8)) + t9
 *   cost(a -> b) "remove a, keep b where it is" = value(Q[a] + Q[b] entry by entry, p_b) if that is > 0, else +0.
 *
 * CANDIDATES, one lane per edge e = (lo, hi).  cost[e] = (cost(lo -> hi), cost(hi -> lo)) is stored for every edge.  Only
 *   an interior edge is a candidate.  The direction of the smaller cost is tried first, lo -> hi on equal cost, then the
 *   other; dir[e] = 0 (none), 1 (remove lo) or 2 (remove hi).  a -> b is allowed when, tested in this order:
 *     bnd[a] = 0 (the kept vertex b may lie on the boundary);
 *     |nbr(a) & nbr(b)| = 2 (the link condition);
 *     each of those two vertices n has deg(n) > 3, or > 2 if bnd[n] (without this guard a tetrahedron, an octahedron and
 *       every closed mesh end in pairs of coincident faces);
 *     every corner of a (ascending) whose face does not name b has dot(N(old), N(with p_a replaced by p_b)) > 0 in fp64,
 *       N as above over the face's corners in their stored order, dot(m, n) = (m.x n.x + m.y n.y) + m.z n.z.
 *   There is no length guard.  key[e] = ((bits of (float) cost of the chosen direction) << 32) | e, a signed 64-bit integer
 *   that is >= 0; INT64_MAX for an edge that is no candidate, so that a signed sort puts those last.
 *
 * ROUND on one connectivity of F faces towards `target`:  m = ceil((F - target) / 2).  The caller sorts key; the threshold
 *   is sorted[min(m, E) - 1], handed on as a device pointer.  LIVE are the candidates with key <= threshold: at most m, and
 *   a collapse removes two faces, so a round ends with F >= target - 1.  lock [V] starts at 0, remap [V] at the identity.
 *   `passes` times, vkey [V] preset to all ones by the caller each time:
 *     spread   a live candidate none of whose ring vertices R(e) = {lo, hi} + nbr(lo) + nbr(hi) is locked takes
 *              atomicMin(key) onto every vertex of R(e);
 *     select   a live candidate that finds its key on every vertex of R(e) is selected: remap[a] = b, Q[b] = Q[b] + Q[a]
 *              entry by entry, lock = 1 on R(e), FLAG_SELECTED += 1.  (A candidate that did not spread finds its key nowhere:
 *              keys are distinct.  So select reads no lock and the locks written in a pass are read only by the next.)
 *   Then gd_mesh_remesh_relabel and gd_mesh_remesh_compact_faces.
 *   DISJOINTNESS.  Within a pass every vertex holds one key, so two selected candidates have disjoint rings.  A candidate
 *   selected in a later pass spread, so its ring holds no locked vertex, so it is disjoint from the ring of every earlier
 *   winner.  A collapse a -> b changes: the faces of a (all their vertices lie in its ring), the neighbour rows and degrees
 *   of vertices of its ring, Q[b], and nothing else -- no position ever changes, the kept vertex stays where it is.  What a
 *   later winner a' -> b' reads -- the rows of a' and b', the degrees of their two common neighbours, the faces of a',
 *   positions, Q[a'] and Q[b'], dir and key computed before the first pass -- belongs to vertices of its own ring or to
 *   faces that name a', none of them in an earlier ring.  So every winner's tests hold on the mesh as the earlier winners
 *   left it, remap has no chains (b is locked and never removed later in the round), and no face names two removed vertices.
 *
 * TERMINATION is the caller's: F <= target (then target - 1 <= F <= target), a round that selected nothing, or the round
 *   limit.  Consequence of bnd[a] = 0: the boundary's vertices, positions and edges come back exactly.
 *
 * TAUBIN SMOOTHING, fp32, Jacobi: one launch is one pass with weight w,  out = p + w (mean - p)  per component with
 *   mean = s / (float) k,  s = the sum of p_n, from 0, over the counted neighbours n of v in ascending order, k their number.
 *   An interior vertex counts every neighbour; a vertex with bnd = 1 counts the neighbours it is joined to by a boundary
 *   edge (the rim smooths along itself and does not shrink inward); k = 0: out = p.  A step is a pass with w = lambda and a
 *   pass with w = mu; MeshLab documents lambda = 0.5, mu = -0.53 and 10 steps for apply_coord_taubin_smoothing.
 *
 * ROTATE: out = (x, z, -y), the rotation by -90 degrees about x, exactly.
 */
#ifndef GD_MESH_SIMPLIFY_H_INCLUDED
#define GD_MESH_SIMPLIFY_H_INCLUDED

#include "gd_mesh_remesh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Q [V][10] */
int gd_mesh_simplify_quadrics(void* stream, const gd_remesh_mesh* mesh, double* Q);
/* key [E], dir [E], cost [E][2] */
int gd_mesh_simplify_candidates(void* stream, const gd_remesh_mesh* mesh, const double* Q, int64_t* key, int* dir,
                                double* cost);
/* threshold: one device word; lock [V]; vkey [V] preset to all ones */
int gd_mesh_simplify_spread(void* stream, const gd_remesh_mesh* mesh, const int64_t* key, const int64_t* threshold,
                            const int* lock, uint64_t* vkey);
int gd_mesh_simplify_select(void* stream, const gd_remesh_mesh* mesh, const int64_t* key, const int64_t* threshold,
                            const int* dir, const uint64_t* vkey, int* remap, double* Q, int* lock, int* flags);
/* verts_out [V][3], not mesh->verts */
int gd_mesh_simplify_smooth(void* stream, const gd_remesh_mesh* mesh, float w, float* verts_out);
int gd_mesh_simplify_rotate(void* stream, int V, const float* verts, float* verts_out);

#ifdef __cplusplus
}
#endif
#endif
