/*
 * gd_mesh_deform.h -- C-ABI of the moving-geometry side of the mesh render path (stage 3, the mesh deformer:
 * Garment_Deformer_NeTF/deformer/core/renderer.py:104-164), exported by libgd_raster.so (csrc/raster_mesh.hip).  The
 * forward entries and the DEFINITIONS of every gradient here are in gd_mesh.h; this header adds nvdiffrast's rast_db
 * path, the position gradient of antialias, and the visible-vertex mask.
 *
 * Same contract as gd_mesh.h: plain device pointers, caller's HIP stream, caller-owned scratch, no host synchronisation,
 * every output element written, reruns bit-identical (no floating-point atomics).  Both position gradients have the
 * shape of gd_mesh_interpolate_backward: one wave per triangle walks the triangle's pixel box (recomputed from pos),
 * keeps the pixels whose rast id is this triangle, reduces in a fixed tree into a [F][3][4] corner slab (the scratch),
 * and one thread per (vertex, component) sums the vertex's corners in the order of corner_idx.  A contribution of the
 * rasterize backward belongs to the corners of the pixel's own triangle; one of an antialias pair to two corners of
 * the chosen triangle, which is the id at pixel I.
 *
 * Return 0 on success, negative on error (gd_mesh_last_error()).
 */
#ifndef GD_MESH_DEFORM_H_INCLUDED
#define GD_MESH_DEFORM_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* drast[H][W][4] = (sum_k dout_k (a0_k - a2_k), sum_k dout_k (a1_k - a2_k), 0, 0), zeros on background.
 * attr: float [V][C], 1 <= C <= GD_MESH_MAX_CHANNELS; dout: float [H][W][C]. */
int gd_mesh_interpolate_backward_rast(void* stream, int V, int F, int C, int H, int W, const float* attr,
                                      const float* rast, const int* tri, const float* dout, float* drast);

/* bytes of device scratch gd_mesh_rasterize_backward needs: the [F][3][4] corner slab */
size_t gd_mesh_rasterize_backward_scratch_bytes(int F);

/* dpos[V][4] = (dx, dy, 0, dw) from drast[H][W][4] (channels 2 and 3 ignored).  pos / tri / rast: what
 * gd_mesh_rasterize took and returned; corner_ptr / corner_idx as in gd_mesh_interpolate_backward. */
int gd_mesh_rasterize_backward(void* stream, int V, int F, int H, int W, const float* pos, const int* tri,
                               const float* rast, const float* drast, const int* corner_ptr, const int* corner_idx,
                               float* dpos, void* scratch);

/* bytes of device scratch gd_mesh_antialias_backward_pos needs: the [F][3][4] corner slab */
size_t gd_mesh_antialias_backward_pos_scratch_bytes(int F);

/* dpos[V][4] = (dx, dy, 0, dw) of out = antialias(in) with the upstream gradient dout; in / dout: float [H][W][C],
 * any C >= 1.  The pairs' decisions come from the device function gd_mesh_antialias_weights uses.  The gradient to
 * `in` is gd_mesh_antialias_apply with adjoint != 0. */
int gd_mesh_antialias_backward_pos(void* stream, int V, int F, int C, int H, int W, const float* rast, const float* pos,
                                   const int* tri, const int* opp, const float* in, const float* dout,
                                   const int* corner_ptr, const int* corner_idx, float* dpos, void* scratch);

/* vis[tri[id - 1][i]] = 1 for every pixel of rast (float [npix][4]) with id > 0: plain byte stores of the constant 1.
 * vis: uint8 [V], zeroed by the caller, so that one call per view accumulates the union. */
int gd_mesh_visible_vertices(void* stream, int V, int F, int npix, const float* rast, const int* tri, uint8_t* vis);

#ifdef __cplusplus
}
#endif
#endif
