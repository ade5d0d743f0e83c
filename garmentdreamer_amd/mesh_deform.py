"""Mesh render path for MOVING geometry: what stage 3 of the reference, the mesh deformer, rests on
(Garment_Deformer_NeTF/deformer/core/renderer.py:104-164; ``deformation.py`` runs Adam on vertex offsets through it), on
the HIP kernels of ``csrc/raster_mesh.hip`` (C-ABI: include/gd_mesh_deform.h; definitions: include/gd_mesh.h) -- no CPU
path.  ``mesh_render`` keeps the fixed-geometry ops, which refuse positions that require a gradient; the ops here have the
same forward, bit for bit, and add the gradients to vertex positions:

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

from . import _native
from . import mesh_render as _mr
from .mesh_render import MAX_CHANNELS, MeshTopology, _check, _gpu, _stream, _unbatch, build_topology  # noqa: F401


def _topology(name: str, topology: Optional[MeshTopology], tri: torch.Tensor, V: int) -> MeshTopology:
    if topology is None:
        return build_topology(tri, num_vertices=V, device=tri.device)
    if not topology.corner_ptr.is_cuda or topology.corner_ptr.shape[0] != V + 1 \
            or topology.corner_idx.shape[0] != 3 * tri.shape[0] or tuple(topology.opp.shape) != tuple(tri.shape):
        raise ValueError(f"{name}: topology does not belong to this mesh (or is not on the GPU)")
    return topology


def _scratch(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, tri, H, W, topology):
        rast = _mr.rasterize(pos.detach(), tri, (H, W))
        ctx.save_for_backward(pos, tri, rast)
        ctx.topology = topology
        return rast

    @staticmethod
    def backward(ctx, drast):
        pos, tri, rast = ctx.saved_tensors
        dev = pos.device
        H, W = rast.shape[:2]
        V, nf = pos.shape[0], tri.shape[0]
        L = _native.lib()
        drast = drast.contiguous()
        dpos = torch.empty((V, 4), dtype=torch.float32, device=dev)
        scratch = _scratch(L.gd_mesh_rasterize_backward_scratch_bytes(nf), dev)
        with torch.cuda.device(dev):
            _check(L.gd_mesh_rasterize_backward(_stream(dev), V, nf, H, W, pos.data_ptr(), tri.data_ptr(),
                                                rast.data_ptr(), drast.data_ptr(), ctx.topology.corner_ptr.data_ptr(),
                                                ctx.topology.corner_idx.data_ptr(), dpos.data_ptr(), scratch.data_ptr()),
                   "gd_mesh_rasterize_backward")
        return dpos, None, None, None, None


def rasterize(pos: torch.Tensor, tri: torch.Tensor, resolution, topology: Optional[MeshTopology] = None) -> torch.Tensor:
    """``rast`` float32 [H,W,4] = (u, v, z/w, triangle id + 1) exactly as ``mesh_render.rasterize`` returns it, with an
    autograd edge to ``pos`` (float32 clip-space [V,4] or [1,V,4]): the gradient of ``rast[..., 0:2]`` reaches x, y and w
    of the covering triangle's corners; channels 2 and 3 pass none on.  ``topology``: ``build_topology(tri)``, built here
    if missing (a host pass over the mesh)."""
    _gpu("rasterize", "pos", pos, torch.float32, 4)
    _gpu("rasterize", "tri", tri, torch.int32, 3)
    p, batched = _unbatch("rasterize", "pos", pos, 2)
    if tri.dim() != 2:
        raise ValueError("rasterize: tri must be [F,3]")
    H, W = int(resolution[0]), int(resolution[1])
    t = tri.contiguous()
    if p.requires_grad and torch.is_grad_enabled():
        rast = _Rasterize.apply(p.contiguous(), t, H, W, _topology("rasterize", topology, t, p.shape[0]))
    else:
        rast = _mr.rasterize(p.detach(), t, (H, W))
    return rast[None] if batched else rast


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, tri, pos, topology):
        dev = attr.device
        H, W = rast.shape[:2]
        V, C = attr.shape
        out = torch.empty((H, W, C), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _check(_native.lib().gd_mesh_interpolate_forward(_stream(dev), V, tri.shape[0], C, H, W, attr.data_ptr(),
                                                             rast.data_ptr(), tri.data_ptr(), out.data_ptr()),
                   "gd_mesh_interpolate_forward")
        ctx.save_for_backward(attr, rast, tri, pos)
        ctx.topology = topology
        return out

    @staticmethod
    def backward(ctx, dout):
        attr, rast, tri, pos = ctx.saved_tensors
        dev = rast.device
        H, W = rast.shape[:2]
        V, C = attr.shape
        nf = tri.shape[0]
        L = _native.lib()
        dout = dout.contiguous()
        dattr = drast = None
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0]:
                dattr = torch.empty((V, C), dtype=torch.float32, device=dev)
                scratch = _scratch(L.gd_mesh_interpolate_backward_scratch_bytes(nf, C), dev)
                _check(L.gd_mesh_interpolate_backward(_stream(dev), V, nf, C, H, W, pos.data_ptr(), tri.data_ptr(),
                                                      rast.data_ptr(), dout.data_ptr(),
                                                      ctx.topology.corner_ptr.data_ptr(),
                                                      ctx.topology.corner_idx.data_ptr(), dattr.data_ptr(),
                                                      scratch.data_ptr()), "gd_mesh_interpolate_backward")
            if ctx.needs_input_grad[1]:
                drast = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
                _check(L.gd_mesh_interpolate_backward_rast(_stream(dev), V, nf, C, H, W, attr.data_ptr(), rast.data_ptr(),
                                                           tri.data_ptr(), dout.data_ptr(), drast.data_ptr()),
                       "gd_mesh_interpolate_backward_rast")
        return dattr, drast, None, None, None


def interpolate(attr: torch.Tensor, rast: torch.Tensor, tri: torch.Tensor, pos: torch.Tensor,
                topology: Optional[MeshTopology] = None) -> torch.Tensor:
    """``out`` [H,W,C] = (u a0 + v a1) + (1 - u - v) a2 as ``mesh_render.interpolate``, differentiable in ``attr``
    (float32 [V,C], C <= 8) and in ``rast`` (which ``rasterize`` above carries on to the positions).  ``pos``: the
    positions ``rast`` was made from (the gradient to ``attr`` walks each triangle's pixel box again); it receives no
    gradient from this op itself."""
    _gpu("interpolate", "attr", attr, torch.float32, None)
    _gpu("interpolate", "rast", rast, torch.float32, 4)
    _gpu("interpolate", "tri", tri, torch.int32, 3)
    _gpu("interpolate", "pos", pos, torch.float32, 4)
    a, b1 = _unbatch("interpolate", "attr", attr, 2)
    r, b2 = _unbatch("interpolate", "rast", rast, 3)
    p = _unbatch("interpolate", "pos", pos.detach(), 2)[0].contiguous()
    if not 1 <= a.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"interpolate: attr must have 1..{MAX_CHANNELS} channels")
    if p.shape[0] != a.shape[0]:
        raise ValueError("interpolate: pos and attr must have one row per vertex")
    t = tri.contiguous()
    if topology is not None or (a.requires_grad and torch.is_grad_enabled()):
        topology = _topology("interpolate", topology, t, a.shape[0])
    out = _Interpolate.apply(a.contiguous(), r.contiguous(), t, p, topology)
    return out[None] if (b1 or b2) else out


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, pos, rast, tri, topology, wts):
        ctx.save_for_backward(color, pos, rast, tri, wts)
        ctx.topology = topology
        return _mr._aa_apply(color, wts, False)

    @staticmethod
    def backward(ctx, dout):
        color, pos, rast, tri, wts = ctx.saved_tensors
        dout = dout.contiguous()
        dcolor = _mr._aa_apply(dout, wts, True) if ctx.needs_input_grad[0] else None
        dpos = None
        if ctx.needs_input_grad[1]:
            dev = pos.device
            H, W, C = color.shape
            V, nf = pos.shape[0], tri.shape[0]
            topo = ctx.topology
            L = _native.lib()
            dpos = torch.empty((V, 4), dtype=torch.float32, device=dev)
            scratch = _scratch(L.gd_mesh_antialias_backward_pos_scratch_bytes(nf), dev)
            with torch.cuda.device(dev):
                _check(L.gd_mesh_antialias_backward_pos(_stream(dev), V, nf, C, H, W, rast.data_ptr(), pos.data_ptr(),
                                                        tri.data_ptr(), topo.opp.data_ptr(), color.data_ptr(),
                                                        dout.data_ptr(), topo.corner_ptr.data_ptr(),
                                                        topo.corner_idx.data_ptr(), dpos.data_ptr(), scratch.data_ptr()),
                       "gd_mesh_antialias_backward_pos")
        return dcolor, dpos, None, None, None, None


def antialias(color: torch.Tensor, rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor,
              topology: Optional[MeshTopology] = None, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dr.antialias``: the blend of ``mesh_render.antialias``, differentiable in ``color`` [H,W,C] and in ``pos``: a
    silhouette edge that moves changes how much of the neighbouring pixel is blended in, which is the only way a mask
    reaches the vertices.  ``weights=mesh_render.antialias_weights(rast, pos.detach(), tri, topology)`` shares the
    analysis between images of one (rast, pos); each image still gets its own gradient to ``pos``, because that gradient
    is computed from the image and its upstream gradient, not from the shared weights."""
    _gpu("antialias", "color", color, torch.float32, None)
    _gpu("antialias", "rast", rast, torch.float32, 4)
    _gpu("antialias", "pos", pos, torch.float32, 4)
    _gpu("antialias", "tri", tri, torch.int32, 3)
    c, batched = _unbatch("antialias", "color", color, 3)
    r = _unbatch("antialias", "rast", rast.detach(), 3)[0].contiguous()
    p = _unbatch("antialias", "pos", pos, 2)[0].contiguous()
    t = tri.contiguous()
    topology = _topology("antialias", topology, t, p.shape[0])
    topology = MeshTopology(topology.opp.contiguous(), topology.corner_ptr.contiguous(), topology.corner_idx.contiguous())
    if weights is None:
        weights = _mr.antialias_weights(r, p.detach(), t, topology)
    else:
        _gpu("antialias", "weights", weights, torch.float32, 4)
    if tuple(r.shape[:2]) != tuple(c.shape[:2]) or tuple(weights.shape) != (c.shape[0], c.shape[1], 4):
        raise ValueError("antialias: rast and weights must be [H,W,4] of the colour's resolution")
    out = _Antialias.apply(c.contiguous(), p, r, t, topology, weights.detach().contiguous())
    return out[None] if batched else out


def visible_vertices(rasts, tri: torch.Tensor, num_vertices: int) -> torch.Tensor:
    """bool [V]: True for the vertices of every triangle that won at least one pixel of ``rasts`` (one ``rast`` or a
    sequence of them, any resolutions): the reference's ``cat`` / ``unique`` / ``unique`` over the id images
    (renderer.py:104-126) as one launch per image that stores ones."""
    if isinstance(rasts, torch.Tensor):
        rasts = [rasts]
    _gpu("visible_vertices", "tri", tri, torch.int32, 3)
    if tri.dim() != 2:
        raise ValueError("visible_vertices: tri must be [F,3]")
    t = tri.contiguous()
    dev = t.device
    V = int(num_vertices)
    vis = torch.zeros(max(V, 1), dtype=torch.uint8, device=dev)
    L = _native.lib()
    for rast in rasts:
        _gpu("visible_vertices", "rast", rast, torch.float32, 4)
        r = _unbatch("visible_vertices", "rast", rast.detach(), 3)[0].contiguous()
        with torch.cuda.device(dev):
            _check(L.gd_mesh_visible_vertices(_stream(dev), V, t.shape[0], r.shape[0] * r.shape[1], r.data_ptr(),
                                              t.data_ptr(), vis.data_ptr()), "gd_mesh_visible_vertices")
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
        _gpu("GBufferRenderer", "vertices", vertices, torch.float32, 3)
        if not isinstance(indices, torch.Tensor) or not indices.is_cuda:
            raise RuntimeError("GBufferRenderer: the HIP kernels have no CPU path (indices must be on the GPU)")
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
            _gpu("GBufferRenderer", "vertex_normals", vertex_normals, torch.float32, 3)
        mvps, resolutions = self._views(mvps, resolutions)
        topo = _topology("GBufferRenderer", topology, idx, vertices.shape[0])
        gbuffers = []
        for mvp, res in zip(mvps, resolutions):
            gbuffer = {}
            pos = self.transform_pos(mvp, vertices)
            rast = rasterize(pos, idx, res, topo)
            wts = _mr.antialias_weights(rast.detach(), pos.detach(), idx, topo) if with_antialiasing else None

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
