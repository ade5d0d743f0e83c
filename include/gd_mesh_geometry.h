/*
 * gd_mesh_geometry.h -- C-ABI and DEFINITIONS of the mesh deformer's geometry terms (stage 3 of the reference:
 * Garment_Deformer_NeTF/deformer/core/mesh.py compute_normals, losses/laplacian.py, losses/normal_consistency.py,
 * utils/geometry.py), exported by libgd_raster.so (csrc/raster_geometry.hip): face and vertex normals of a moving mesh,
 * the uniform Laplacian loss and the normal-consistency loss, each with its backward.
 *
 * Same contract as gd_mesh.h: plain device pointers, caller's HIP stream, caller-owned scratch with a *_scratch_bytes
 * query, no host synchronisation, every output element written, no floating-point atomics, reruns bit-identical.  All
 * arithmetic is fp32 in the order written below (the file is built with -ffp-contract=off).  Every entry validates its
 * arguments before any device work: a null pointer, V <= 0 or F < 0 returns -1 with a message in gd_mesh_last_error().
 * Return 0 on success, -1 on a bad call, -2 on a HIP error.
 *
 * Host-built index arrays (mesh_geometry.build_geometry), all int32:
 *   tri        [F][3]   corners a, b, c of each face
 *   corner_ptr [V+1], corner_idx [3F]   the CSR of mesh_render.build_topology: the corners k = 3 f + i of each vertex,
 *                       ascending; corner k belongs to face k / 3
 *   nbr_ptr    [V+1], nbr_idx [N]       N(i): the vertices sharing an edge with i, ascending, each once; N = 2 E;
 *                       deg_i = nbr_ptr[i+1] - nbr_ptr[i]; the adjacency is symmetric
 *   face_nbr   [F][3]   the face across edge i of face f (edge i runs between corners i+1 and i+2), or -1 unless exactly
 *                       two faces share that edge.  Two faces that share three edges (duplicates) name each other
 *                       three times.  A face that lists a vertex twice never names itself.
 * An index outside its range is never followed: such a face has fn = 0 and passes no gradient, such a neighbour is
 * skipped.
 *
 * NORMALS.  dot(p, q) = (p.x q.x + p.y q.y) + p.z q.z and |p| = sqrtf(dot(p, p)) throughout.
 *   forward   c_f = (b - a) x (c - a), component by component u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x;
 *             fn_f = c_f / max(|c_f|, 1e-12)           (torch.nn.functional.normalize, eps 1e-12)
 *             s_v  = sum of fn_{k/3} over the corners k of v in the order of corner_idx, starting from 0
 *             len_v = |s_v|,  vn_v = s_v / max(len_v, 1e-12)   (a vertex without a corner: len = 0, vn = 0)
 *   backward  N(x, n, l, g), the adjoint of n = x / max(l, 1e-12) with l = |x|:
 *                 l > 1e-12:  (g - n dot(n, g)) / l          otherwise:  g / 1e-12   (the clamp's branch, as torch has it)
 *             per face: G = dfn_f + N(s_a, vn_a, len_a, dvn_a) + N(.. b ..) + N(.. c ..), added in this order (a null dfn
 *             or dvn stands for zeros), then Gc = N(c_f, fn_f, |c_f|, G) and with u = b - a, w = c - a:
 *                 du = w x Gc,  dw = Gc x u,  corner gradients  a: (-du) - dw,  b: du,  c: dw
 *             stored as (x, y, z, 0) in a [F][3][4] slab (the scratch); dverts_v = sum of its corners' rows in the order
 *             of corner_idx, starting from 0 (exactly 0 for a vertex without a corner).
 *
 * UNIFORM LAPLACIAN.  delta_i = (sum_{j in N(i)} v_j, ascending, from 0) / (float)deg_i - v_i per component, and
 *   delta_i = -v_i where deg_i = 0 (what the reference's matrix does to an isolated vertex).
 *   loss = (sum_i dot(delta_i, delta_i)) / (float)V.  The sum: workgroup b adds the 256 values of vertices 256 b ...
 *   256 b + 255 (0 beyond V) in a binary tree (stride 128, 64, ..., 1: x[t] += x[t + stride]) into a partial; one workgroup
 *   then gives thread t the partials t, t + 256, ... added in that order from 0 and reduces the 256 results in the same
 *   tree.
 *   backward  dv_k = (dloss (2 / (float)V)) ((sum_{j in N(k)} delta_j / (float)deg_j, ascending, from 0) - delta_k);
 *   dloss is read from device memory.
 *
 * NORMAL CONSISTENCY.  For faces f, g:  m_f = max(|fn_f|, 1e-8),  cos = dot(fn_f, fn_g) / (m_f m_g)
 *   (torch.cosine_similarity, eps 1e-8), term = (1 - cos)^2.  A pair is an (f, i) with face_nbr[f][i] = g > f; P is their
 *   number, given by the caller.  loss = (sum of the terms) / (float)P, the terms of face f added in edge order from 0 and
 *   the faces' sums reduced as above; P = 0 gives loss = 0 and dfn = 0 (the reference's mean over nothing is NaN).
 *   backward  dfn_f = sum over i with g = face_nbr[f][i] >= 0, g != f, in edge order from 0, of
 *                 ((dloss / (float)P) (-2 (1 - cos))) D,   D = (fn_g / m_g - [|fn_f| > 1e-8] cos fn_f / m_f) / m_f
 *   (every pair reaches both of its faces; dloss is read from device memory).
 */
#ifndef GD_MESH_GEOMETRY_H_INCLUDED
#define GD_MESH_GEOMETRY_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* fn: float [F][3], vn: float [V][3], len: float [V] (|s_v|, what the backward reads).  verts: float [V][3].
 * Two launches: one thread per face, one thread per vertex. */
int gd_mesh_normals_forward(void* stream, int V, int F, const float* verts, const int* tri, const int* corner_ptr,
                            const int* corner_idx, float* fn, float* vn, float* len);

/* bytes of device scratch gd_mesh_normals_backward needs: the [F][3][4] corner slab (0 for F < 0) */
size_t gd_mesh_normals_backward_scratch_bytes(int F);

/* dverts: float [V][3].  vn / len: what the forward returned for these verts; dvn: float [V][3] or NULL; dfn: float
 * [F][3] or NULL.  Two launches: one thread per face, one thread per vertex. */
int gd_mesh_normals_backward(void* stream, int V, int F, const float* verts, const int* tri, const int* corner_ptr,
                             const int* corner_idx, const float* vn, const float* len, const float* dvn,
                             const float* dfn, float* dverts, void* scratch);

/* bytes of device scratch of the two loss forwards: the per-workgroup partials of n elements (0 for n < 0) */
size_t gd_mesh_loss_scratch_bytes(int n);

/* delta: float [V][3] (what the backward reads), loss: float [1].  N: the length of nbr_idx.  scratch:
 * gd_mesh_loss_scratch_bytes(V).  Two launches. */
int gd_mesh_laplacian_forward(void* stream, int V, int N, const float* verts, const int* nbr_ptr, const int* nbr_idx,
                              float* delta, float* loss, void* scratch);

/* dverts: float [V][3]; dloss: float [1] on the device.  One launch. */
int gd_mesh_laplacian_backward(void* stream, int V, int N, const int* nbr_ptr, const int* nbr_idx, const float* delta,
                               const float* dloss, float* dverts);

/* loss: float [1].  P >= 0: the number of pairs.  scratch: gd_mesh_loss_scratch_bytes(F).  Two launches. */
int gd_mesh_normal_consistency_forward(void* stream, int F, int P, const float* fn, const int* face_nbr, float* loss,
                                       void* scratch);

/* dfn: float [F][3]; dloss: float [1] on the device.  One launch. */
int gd_mesh_normal_consistency_backward(void* stream, int F, int P, const float* fn, const int* face_nbr,
                                        const float* dloss, float* dfn);

#ifdef __cplusplus
}
#endif
#endif
