/*
 * gd_fit.h -- C-ABI and DEFINITIONS of the loss head of the NeTF stage's texture fit (the tail of Renderer.render and the
 * masked MSE of Renderer.fit_texture_from_mesh, Garment_Deformer_NeTF/netf/render/mesh_renderer.py:158-240 and :376-428),
 * exported by libgd_raster.so (csrc/raster_fit.hip).  One view per call.
 *
 * Same contract as gd_mesh_losses.h: plain device pointers, caller's HIP stream, caller-owned scratch with a
 * *_scratch_bytes query, no host synchronisation, every output element written, no floating-point atomics, no wait on
 * another workgroup, reruns bit-identical.  All arithmetic is fp32 in the order written below (the file is built with
 * -ffp-contract=off; division and sqrtf are correctly rounded).  Every entry validates its arguments before any device
 * work: a null pointer, H <= 0, W <= 0, H W >= 2^30 or an image pointer that is not 16-byte aligned returns -1 with a
 * message in gd_mesh_last_error().  Return 0 on success, -1 on a bad call, -2 on a HIP error.
 *
 * Buffers of a view, all float, pixel i = y W + x:
 *   c_aa [H][W][3]          antialiased colour, before the clamp
 *   a_aa [H][W]             antialiased alpha, before its second clamp
 *   p_aa, n_aa [H][W][3]    antialiased position and unnormalised normal
 *   center [3]              the camera's centre, world space; device memory
 *   rgb [H][W][3], tmask [H][W]   the target view's image and mask
 *   bg [3]                  the background colour; device memory
 *   flip_rows               if not 0 the target pixel of (y, x) is j = (H - 1 - y) W + x (the reference's torch.flipud),
 *                           else j = i
 *
 * PER PIXEL.  dot(p, q) = (p.x q.x + p.y q.y) + p.z q.z and |p| = sqrtf(dot(p, p)).
 *   a       = min(max(a_aa, 0), 1)
 *   c_k     = min(max(c_aa_k, 0), 1)                                        per channel k
 *   image_k = a c_k + (1 - a) bg_k     four roundings: u = 1 - a, s = a c_k, t = u bg_k, image_k = s + t
 *   d       = p_aa - center,  d = d / max(|d|, 1e-12) per component         (torch's F.normalize)
 *   cos     = dot(d, n_aa) / (max(|d|, 1e-6) max(|n_aa|, 1e-6))             (|d| of the normalised d; torch's
 *                                                                            cosine_similarity with eps 1e-6)
 *   m       = a > 0 and tmask[j] > 0 and cos <= 0
 *   e       = (r_0 r_0 + r_1 r_1) + r_2 r_2,  r_k = image_k - rgb[j]_k      where m, else e = 0
 * A NaN compares false: a NaN alpha or cosine leaves the pixel out.
 *
 * LOSS.  count = the number of pixels with m (int32), sum = the sum of e in the order below, and
 *   loss = sum / (3 (float)count)        if count > 0, else 0 and a zero gradient
 * which is the reference's MSELoss over image[m] and flipud(rgb)[m].  The one deviation: for an empty selection the
 * reference's mean over nothing is NaN.
 *
 * SUMS.  Pixels are taken GD_FIT_PIXELS_PER_PARTIAL = 256 at a time (e = 0 beyond H W).  Within such a group lane l of 64
 * holds the GD_FIT_PIXELS_PER_LANE = 4 consecutive pixels 4 l ... 4 l + 3 and adds their e in that order,
 * q_l = ((e_0 + e_1) + e_2) + e_3; the 64 q are then reduced in a binary tree (stride 32, 16, ..., 1: x[l] += x[l + stride]
 * for l < stride) into the group's partial.  One workgroup of GD_FIT_FINAL_THREADS = 256 threads then gives thread t the
 * partials t, t + 256, t + 512, ... added in that order from 0 and reduces the 256 results in the same kind of tree (stride
 * 128, ..., 1).  The counts go the same way in int32.  The longest chain of additions a term passes through is therefore
 * 2 (channels) + 3 (lane) + 6 (tree) + ceil(partials / 256) (thread) + 8 (tree).
 *
 * BACKWARD, towards c_aa only (a_aa, p_aa, n_aa and the targets carry no gradient: the geometry is fixed).  With
 *   g = count > 0 ? (2 dloss) / (3 (float)count) : 0        (dloss and count read from device memory)
 *   dc_aa_k = (g r_k) a     where m and 0 <= c_aa_k <= 1 (inclusive, as torch's clamp backward), else 0
 * image is recomputed as above; m is the forward's.
 *
 * stats: GD_FIT_STATS_WORDS = 4 words.  float loss; int32 count; float sum; 0.
 */
#ifndef GD_FIT_H_INCLUDED
#define GD_FIT_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#define GD_FIT_PIXELS_PER_LANE 4
#define GD_FIT_PIXELS_PER_PARTIAL 256
#define GD_FIT_FINAL_THREADS 256
#define GD_FIT_STATS_WORDS 4

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device scratch of the forward: one {sum, count} partial per 256 pixels (0 for pixels <= 0) */
size_t gd_fit_loss_scratch_bytes(int64_t pixels);

/* image: float [H][W][3], cosinesview: float [H][W], m: uint8 [H][W] (0 or 1), stats: 4 words, see above.  Two launches:
 * one lane per four pixels with one partial per wave, then one workgroup over the partials. */
int gd_fit_loss_forward(void* stream, int H, int W, int flip_rows, const float* c_aa, const float* a_aa, const float* p_aa,
                        const float* n_aa, const float* center, const float* rgb, const float* tmask, const float* bg,
                        float* image, float* cosinesview, uint8_t* m, void* stats, void* scratch);

/* dc_aa: float [H][W][3].  m, stats: what the forward wrote for these inputs; dloss: float [1] on the device.  One launch,
 * one lane per four pixels. */
int gd_fit_loss_backward(void* stream, int H, int W, int flip_rows, const float* c_aa, const float* a_aa, const float* rgb,
                         const float* bg, const uint8_t* m, const void* stats, const float* dloss, float* dc_aa);

#ifdef __cplusplus
}
#endif
#endif
