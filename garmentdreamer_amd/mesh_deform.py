"""Mesh render path for MOVING geometry: what stage 3 of the reference, the mesh deformer, rests on
(Garment_Deformer_NeTF/deformer/core/renderer.py:104-164; ``deformation.py`` runs Adam on vertex offsets through it), on
the HIP kernels of ``csrc/raster_mesh.hip`` (C-ABI: include/gd_mesh_deform.h; definitions: include/gd_mesh.h) -- no CPU
path.  ``mesh_render`` keeps the fixed-geometry ops, which refuse positions that require a gradient; the ops here have the
same forward, bit for bit (both modules call the autograd functions of ``_mesh_ops``), and add the gradients to vertex
positions:

  * ``rasterize(pos, tri, resolution, topology)``          ``rast`` with an autograd edge to ``pos`` (nvdiffrast's rast_db
                                                            path: the derivative of the barycentrics (u, v))
  * ``interpolate(attr, rast, tri, pos, topology)``         gradients to ``attr`` and to ``rast``
  * ``antialias(color, rast, pos, tri, topology, weights)`` gradients to ``color`` and to ``pos``
  * ``visible_vertices(rasts, tri, num_vertices)``          bool [V]: the vertices of every triangle that won a pixel
  * ``GBufferRenderer``                                     ``Renderer.render`` / ``get_vert_visibility`` of the deformer

The gradients are those of the forward with the vertex snapping removed and its discrete decisions held fixed (which
triangle a pixel shows; the triangle, edge, side and branch of every antialias pair).  They come without atomics and are
bit-reproducible.  Limits: no near-plane clipping (a triangle with a vertex at ``w <= 0`` is dropped), one image per call
(an optional minibatch axis of 1 is carried through), ``z`` never receives a gradient.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import _mesh_ops as ops
from ._launch import launch, require_gpu
from ._mesh_ops import MeshTopology, build_topology
from .mesh_render import MAX_CHANNELS, antialias_weights  # noqa: F401  (MAX_CHANNELS: a public name of this module too)


def _topology(name: str, topology: Optional[MeshTopology], tri: torch.Tensor, V: int) -> MeshTopology:
    if topology is None:
        return build_topology(tri, num_vertices=V, device=tri.device)
    if not topology.corner_ptr.is_cuda or topology.corner_ptr.shape[0] != V + 1 \
            or topology.corner_idx.shape[0] != 3 * tri.shape[0] or tuple(topology.opp.shape) != tuple(tri.shape):
        raise ValueError(f"{name}: topology does not belong to this mesh (or is not on the GPU)")
    return topology


def rasterize(pos: torch.Tensor, tri: torch.Tensor, resolution, topology: Optional[MeshTopology] = None) -> torch.Tensor:
    """``rast`` float32 [H,W,4] = (u, v, z/w, triangle id + 1) exactly as ``mesh_render.rasterize`` returns it, with an
    autograd edge to ``pos`` (float32 clip-space [V,4] or [1,V,4]): the gradient of ``rast[..., 0:2]`` reaches x, y and w
    of the covering triangle's corners; channels 2 and 3 pass none on.  ``topology``: ``build_topology(tri)``, built here
    if missing (a host pass over the mesh)."""
    require_gpu("rasterize", "pos", pos, torch.float32, 4)
    require_gpu("rasterize", "tri", tri, torch.int32, 3)
    p, batched = ops._unbatch("rasterize", "pos", pos, 2)
    if tri.dim() != 2:
        raise ValueError("rasterize: tri must be [F,3]")
    H, W = int(resolution[0]), int(resolution[1])
    t = tri.contiguous()
    if p.requires_grad and torch.is_grad_enabled():
        rast = ops._Rasterize.apply(p.contiguous(), t, H, W, _topology("rasterize", topology, t, p.shape[0]))
    else:
        rast = ops.rasterize_forward(p.detach().contiguous(), t, H, W)
    return rast[None] if batched else rast


def interpolate(attr: torch.Tensor, rast: torch.Tensor, tri: torch.Tensor, pos: torch.Tensor,
                topology: Optional[MeshTopology] = None) -> torch.Tensor:
    """``out`` [H,W,C] = (u a0 + v a1) + (1 - u - v) a2 as ``mesh_render.interpolate``, differentiable in ``attr``
    (float32 [V,C], C <= 8) and in ``rast`` (which ``rasterize`` above carries on to the positions).  ``pos``: the
    positions ``rast`` was made from (the gradient to ``attr`` walks each triangle's pixel box again); it receives no
    gradient from this op itself."""
    require_gpu("interpolate", "attr", attr, torch.float32)
    require_gpu("interpolate", "rast", rast, torch.float32, 4)
    require_gpu("interpolate", "tri", tri, torch.int32, 3)
    require_gpu("interpolate", "pos", pos, torch.float32, 4)
    a, b1 = ops._unbatch("interpolate", "attr", attr, 2)
    r, b2 = ops._unbatch("interpolate", "rast", rast, 3)
    p = ops._unbatch("interpolate", "pos", pos.detach(), 2)[0].contiguous()
    if not 1 <= a.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"interpolate: attr must have 1..{MAX_CHANNELS} channels")
    if p.shape[0] != a.shape[0]:
        raise ValueError("interpolate: pos and attr must have one row per vertex")
    t = tri.contiguous()
    if topology is not None or (a.requires_grad and torch.is_grad_enabled()):
        topology = _topology("interpolate", topology, t, a.shape[0])
    out = ops._Interpolate.apply(a.contiguous(), r.contiguous(), t, p, topology)
    return out[None] if (b1 or b2) else out


def antialias(color: torch.Tensor, rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor,
              topology: Optional[MeshTopology] = None, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dr.antialias``: the blend of ``mesh_render.antialias``, differentiable in ``color`` [H,W,C] and in ``pos``: a
    silhouette edge that moves changes how much of the neighbouring pixel is blended in, which is the only way a mask
    reaches the vertices.  ``weights=mesh_render.antialias_weights(rast, pos.detach(), tri, topology)`` shares the
    analysis between images of one (rast, pos); each image still gets its own gradient to ``pos``, because that gradient
    is computed from the image and its upstream gradient, not from the shared weights."""
    require_gpu("antialias", "color", color, torch.float32)
    require_gpu("antialias", "rast", rast, torch.float32, 4)
    require_gpu("antialias", "pos", pos, torch.float32, 4)
    require_gpu("antialias", "tri", tri, torch.int32, 3)
    c, batched = ops._unbatch("antialias", "color", color, 3)
    r = ops._unbatch("antialias", "rast", rast.detach(), 3)[0].contiguous()
    p = ops._unbatch("antialias", "pos", pos, 2)[0].contiguous()
    t = tri.contiguous()
    topology = _topology("antialias", topology, t, p.shape[0])
    topology = MeshTopology(topology.opp.contiguous(), topology.corner_ptr.contiguous(), topology.corner_idx.contiguous())
    if weights is None:
        weights = antialias_weights(r, p.detach(), t, topology)
    else:
        require_gpu("antialias", "weights", weights, torch.float32, 4)
    if tuple(r.shape[:2]) != tuple(c.shape[:2]) or tuple(weights.shape) != (c.shape[0], c.shape[1], 4):
        raise ValueError("antialias: rast and weights must be [H,W,4] of the colour's resolution")
    out = ops._Antialias.apply(c.contiguous(), weights.detach().contiguous(), p, r, t, topology)
    return out[None] if batched else out


def visible_vertices(rasts, tri: torch.Tensor, num_vertices: int) -> torch.Tensor:
    """bool [V]: True for the vertices of every triangle that won at least one pixel of ``rasts`` (one ``rast`` or a
    sequence of them, any resolutions): the reference's ``cat`` / ``unique`` / ``unique`` over the id images
    (renderer.py:104-126) as one launch per image that stores ones."""
    if isinstance(rasts, torch.Tensor):
        rasts = [rasts]
    require_gpu("visible_vertices", "tri", tri, torch.int32, 3)
    if tri.dim() != 2:
        raise ValueError("visible_vertices: tri must be [F,3]")
    t = tri.contiguous()
    V = int(num_vertices)
    vis = torch.zeros(max(V, 1), dtype=torch.uint8, device=t.device)
    for rast in rasts:
        require_gpu("visible_vertices", "rast", rast, torch.float32, 4)
        r = ops._unbatch("visible_vertices", "rast", rast.detach(), 3)[0].contiguous()
        launch("gd_mesh_visible_vertices", t.device, V, t.shape[0], r.shape[0] * r.shape[1], r, t, vis)
    return vis[:V].bool()


class GBufferRenderer:
    """``Renderer`` of the mesh deformer (deformer/core/renderer.py): G-buffers of a mesh for a set of views,
    differentiable in the vertices and the vertex normals.  A view is given by its matrix ``to_gl_camera(...)`` and its
    resolution (H, W); the ``depth`` channel (a projection of ``position`` by the view) and the losses are plain torch on
    the caller's side."""

    def __init__(self, near: float = 1, far: float = 1000):
        self.near = near
        self.far = far

    @staticmethod
    def projection(fx, fy, cx, cy, n, f, width, height, device=None) -> torch.Tensor:
        """OpenGL projection from pinhole intrinsics (renderer.py:44-54), float32 [4,4]."""
        return torch.tensor([[2.0 * fx / width, 0, 1.0 - 2.0 * cx / width, 0],
                             [0, 2.0 * fy / height, 1.0 - 2.0 * cy / height, 0],
                             [0, 0, -(f + n) / (f - n), -(2 * f * n) / (f - n)],
                             [0, 0, -1, 0.0]], dtype=torch.float32, device=device)

    @staticmethod
    def to_gl_camera(K, R, t, resolution, n=1000, f=5000) -> torch.Tensor:
        """projection @ gl_transform @ [R | t] (renderer.py:55-78) of a camera with intrinsics ``K`` [3,3], rotation
        ``R`` [3,3] and translation ``t`` [3]; ``resolution`` is (H, W).  The reference passes a camera object with
        these three fields."""
        dev = R.device
        proj = GBufferRenderer.projection(fx=float(K[0, 0]), fy=float(K[1, 1]), cx=float(K[0, 2]), cy=float(K[1, 2]),
                                          n=float(n), f=float(f), width=resolution[1], height=resolution[0], device=dev)
        Rt = torch.eye(4, device=dev)
        Rt[:3, :3] = R
        Rt[:3, 3] = t
        gl_transform = torch.tensor([[1., 0, 0, 0], [0, 1., 0, 0], [0, 0, -1., 0], [0, 0, 0, 1.]], device=dev)
        return proj @ (gl_transform @ Rt)

    @staticmethod
    def transform_pos(mtx, pos: torch.Tensor) -> torch.Tensor:
        """[V,4] clip-space positions of ``pos`` [V,3] under ``mtx`` [4,4] (renderer.py:36-42, without the batch axis)."""
        t_mtx = mtx if torch.is_tensor(mtx) else torch.as_tensor(mtx)
        t_mtx = t_mtx.to(device=pos.device, dtype=pos.dtype)
        posw = torch.cat([pos, torch.ones_like(pos[:, 0:1])], dim=1)
        return torch.matmul(posw, t_mtx.t())

    @staticmethod
    def _views(mvps, resolutions):
        mvps = list(mvps) if not (torch.is_tensor(mvps) and mvps.dim() == 2) else [mvps]
        if len(resolutions) == 2 and not hasattr(resolutions[0], "__len__"):
            resolutions = [resolutions] * len(mvps)
        if len(resolutions) != len(mvps):
            raise ValueError("GBufferRenderer: one resolution (H, W) per view, or one for all")
        return mvps, [(int(r[0]), int(r[1])) for r in resolutions]

    @staticmethod
    def _mesh(vertices, indices):
        require_gpu("GBufferRenderer", "vertices", vertices, torch.float32, 3)
        require_gpu("GBufferRenderer", "indices", indices)
        if vertices.dim() != 2:
            raise ValueError("GBufferRenderer: vertices must be [V,3]")
        return indices.detach().int().contiguous()

    def render(self, mvps, vertices: torch.Tensor, indices: torch.Tensor, vertex_normals: Optional[torch.Tensor],
               resolutions, channels: Sequence[str], with_antialiasing: bool = True,
               topology: Optional[MeshTopology] = None):
        """One dict per view with the requested ``channels`` of ``mask`` [H,W,1], ``position`` [H,W,3] and ``normal``
        [H,W,3] (renderer.py:128-164).  ``mvps``: the views' ``to_gl_camera`` matrices; ``resolutions``: (H, W) per view
        or one for all.  Each view is rasterized once and analysed once for all its channels."""
        idx = self._mesh(vertices, indices)
        if "normal" in channels:
            require_gpu("GBufferRenderer", "vertex_normals", vertex_normals, torch.float32, 3)
        mvps, resolutions = self._views(mvps, resolutions)
        topo = _topology("GBufferRenderer", topology, idx, vertices.shape[0])
        gbuffers = []
        for mvp, res in zip(mvps, resolutions):
            gbuffer = {}
            pos = self.transform_pos(mvp, vertices)
            rast = rasterize(pos, idx, res, topo)
            wts = antialias_weights(rast.detach(), pos.detach(), idx, topo) if with_antialiasing else None

            def aa(x):
                return antialias(x, rast, pos, idx, topo, weights=wts) if with_antialiasing else x

            if "mask" in channels:
                gbuffer["mask"] = aa(torch.clamp(rast[..., -1:], 0, 1))
            if "position" in channels:
                gbuffer["position"] = aa(interpolate(vertices, rast, idx, pos, topo))
            if "normal" in channels:
                gbuffer["normal"] = aa(interpolate(vertex_normals, rast, idx, pos, topo))
            gbuffers.append(gbuffer)
        return gbuffers

    def vertex_visibility(self, mvps, vertices: torch.Tensor, indices: torch.Tensor, resolutions,
                          upsample: int = 8) -> torch.Tensor:
        """``get_vert_visibility`` (renderer.py:104-126): bool [V], the vertices of every triangle that shows in at least
        one view rasterized at ``upsample`` times its resolution."""
        idx = self._mesh(vertices, indices)
        mvps, resolutions = self._views(mvps, resolutions)
        with torch.no_grad():
            rasts = [rasterize(self.transform_pos(mvp, vertices), idx, (res[0] * upsample, res[1] * upsample))
                     for mvp, res in zip(mvps, resolutions)]
            return visible_vertices(rasts, idx, vertices.shape[0])
