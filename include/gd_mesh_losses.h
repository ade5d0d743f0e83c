/*
 * gd_mesh_losses.h -- C-ABI and DEFINITIONS of the G-buffer losses of the mesh deformer's second stage (stage 3 of the
 * reference: Garment_Deformer_NeTF/deformer/losses/normal.py normal_map_loss_enhanced / normal_map_loss and
 * losses/mask.py hole_mask_loss), exported by libgd_raster.so (csrc/raster_gbuffer_losses.hip).  One view per call; the
 * three terms share one pass over the G-buffers.
 *
 * Same contract as gd_mesh_geometry.h: plain device pointers, caller's HIP stream, caller-owned scratch with a
 * *_scratch_bytes query, no host synchronisation, every output element written, no floating-point atomics, reruns
 * bit-identical.  All arithmetic is fp32 in the order written below (the file is built with -ffp-contract=off).  Every entry
 * validates its arguments before any device work: a null pointer, H <= 0, W <= 0, H W >= 2^30 or terms outside
 * GD_MESH_LOSSES_ALL (or 0) returns -1 with a message in gd_mesh_last_error().  Return 0 on success, -1 on a bad call, -2 on
 * a HIP error.
 *
 * Buffers of a view, all float, pixel i = y W + x:
 *   normal, position [H][W][3], mask [H][W]          the G-buffer of the moving mesh (world space)
 *   normal_rf, position_rf, mask_rf                   the same of the frozen reference mesh; read only when HOLE is set
 *   target_normal [H][W][3] in [0,1], target_mask [H][W]   the view's estimated normal map and mask; read only when
 *                                                     ENHANCED or PLAIN is set
 *   camera [12]                                       R row-major [3][3], then center [3]; device memory
 *
 * SHARED.  dot(p, q) = (p.x q.x + p.y q.y) + p.z q.z and |p| = sqrtf(dot(p, p)) throughout.  With Rf = diag(1, -1, -1):
 *   r     = R n,  r_i = dot(R[i], n);       n_cam = (r_0, -r_1, -r_2)                              (= Rf (R n))
 *   t     = 2 T - 1 per component, T the pixel of target_normal
 *   v     = center - p,  l = |v|,  u = v / max(l, 1e-12),  q = R u,  d = (-q_0, q_1, q_2)         (= -Rf (R u))
 *   cos_e(a, b) = dot(a, b) / (max(|a|, e) max(|b|, e))                                            (torch.cosine_similarity)
 *   its adjoint towards b:  C_e(a, b) = (a / max(|a|, e) - [|b| > e] cos_e(a, b) b / max(|b|, e)) / max(|b|, e)
 *   camera-space gradients return to the world by  B(g) = R^T (g_0, -g_1, -g_2),  B(g)_j = (R[0][j] h_0 + R[1][j] h_1) +
 *   R[2][j] h_2 with h = (g_0, -g_1, -g_2).
 *
 * ENHANCED (normal_map_loss_enhanced; epsilon is the reference's argument, float32(-0.1) by default).
 *   e  = 1 - cos_1e-8(t, n_cam)
 *   ct = cos_1e-6(d, t), then ct = 0 where ct > epsilon;   cv = cos_1e-6(d, n_cam);   w = expf(|ct|)
 *   Z  = sum of w over ALL H W pixels (a pixel whose ct was zeroed adds 1)
 *   in:  target_mask > 0 and mask > 0 and cv <= 0 and ct <= epsilon  (ct after the zeroing, as the reference tests it)
 *   loss = (sum over the pixels that are in of e w) / Z
 *   backward: towards n_cam only and through e only (w, Z, cv and position carry none: the reference computes them
 *   under no_grad):  g_cam += -(dloss[0] (w / Z)) C_1e-8(t, n_cam)  at the pixels that are in.
 * PLAIN (normal_map_loss with its default L1).
 *   in:  target_mask > 0 and mask > 0;  count_plain their number
 *   diff_c = 0.5 (n_cam_c + 1) - T_c;   loss = (sum over in of (|diff_0| + |diff_1|) + |diff_2|) / (3 (float)count_plain)
 *   backward: g_cam_c += sign(diff_c) (dloss[1] (0.5 / (3 (float)count_plain))),  sign(0) = 0.
 * HOLE (hole_mask_loss with its default MSE).
 *   s = -1 if cos_1e-6(d, n_cam) < 0 else +1;  s_rf the same from the _rf buffers;  in: mask > 0 and mask_rf > 0;
 *   count_hole their number;  loss = (sum over in of (s - s_rf)^2) / (float)count_hole
 *   backward: the reference overwrites the DATA of the cosine with its sign, so autograd still differentiates the cosine
 *   (a straight-through sign): with k = dloss[2] (2 (s - s_rf) / (float)count_hole) at the pixels that are in,
 *       g_cam += k C_1e-6(d, n_cam)
 *       g_d = k C_1e-6(n_cam, d),  g_u = R^T (-g_d.x, g_d.y, g_d.z),
 *       g_v = l > 1e-12 ? (g_u - u dot(u, g_u)) / l : g_u / 1e-12,     dposition = -g_v
 *   The _rf side receives nothing.
 * g_cam starts from 0 and receives the enabled terms in the order ENHANCED, PLAIN, HOLE; dnormal = B(g_cam).  dposition is
 * exactly 0 unless HOLE is set.  A count of 0 gives loss 0 and no gradient from that term (the reference's mean over
 * nothing is NaN); a term that is not enabled has loss 0 (and Z = 0, count = 0).
 *
 * SUMS.  Six per-pixel values (e w, w, the plain term, the hole term as float; the two "in" flags as int32) are reduced as
 * gd_mesh_geometry.h reduces a loss: workgroup b adds the values of pixels 256 b ... 256 b + 255 (0 beyond H W) in a binary
 * tree (stride 128, 64, ..., 1: x[t] += x[t + stride]) into a partial; one workgroup then gives thread t the partials t,
 * t + 256, ... added in that order from 0 and reduces the 256 results in the same tree.
 *
 * stats: 6 words.  float loss_enhanced, loss_plain, loss_hole, Z;  int32 count_plain, count_hole.
 */
#ifndef GD_MESH_LOSSES_H_INCLUDED
#define GD_MESH_LOSSES_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#define GD_MESH_LOSSES_ENHANCED 1
#define GD_MESH_LOSSES_PLAIN 2
#define GD_MESH_LOSSES_HOLE 4
#define GD_MESH_LOSSES_ALL 7
#define GD_MESH_LOSSES_STATS_WORDS 6

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device scratch of the forward: six partials per 256 pixels (0 for pixels <= 0) */
size_t gd_mesh_gbuffer_losses_scratch_bytes(int64_t pixels);

/* stats: 6 words, see above.  The _rf pointers may be NULL unless HOLE is set; target_normal / target_mask may be NULL
 * if only HOLE is set.  Two launches: one thread per pixel, then one workgroup over the partials. */
int gd_mesh_gbuffer_losses_forward(void* stream, int H, int W, int terms, const float* normal, const float* position,
                                   const float* mask, const float* normal_rf, const float* position_rf,
                                   const float* mask_rf, const float* target_normal, const float* target_mask,
                                   const float* camera, float epsilon, void* stats, void* scratch);

/* dnormal, dposition: float [H][W][3].  stats: what the forward wrote for these inputs; dloss: float [3] on the device
 * (enhanced, plain, hole).  One launch, one thread per pixel; the per-pixel terms are recomputed. */
int gd_mesh_gbuffer_losses_backward(void* stream, int H, int W, int terms, const float* normal, const float* position,
                                    const float* mask, const float* normal_rf, const float* position_rf,
                                    const float* mask_rf, const float* target_normal, const float* target_mask,
                                    const float* camera, float epsilon, const void* stats, const float* dloss,
                                    float* dnormal, float* dposition);

#ifdef __cplusplus
}
#endif
#endif
