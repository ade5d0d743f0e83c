"""Mesh render path of the NeTF stage: the three nvdiffrast operations ``Renderer.render`` rests on
(Garment_Deformer_NeTF/netf/render/mesh_renderer.py:338-428), on the HIP kernels of ``csrc/raster_mesh.hip``
(C-ABI and definitions: include/gd_mesh.h) -- no CPU path.  The autograd functions and the topology are in ``_mesh_ops``,
shared with ``mesh_deform``; this module is the fixed-geometry policy over them: ``pos`` and ``rast`` are detached.

  * ``rasterize(pos, tri, resolution)``                    <- ``dr.rasterize``   (no GL context; returns ``rast`` only)
  * ``interpolate(attr, rast, tri)``                        <- ``dr.interpolate`` (gradient to ``attr``)
  * ``antialias(color, rast, pos, tri, topology, weights)`` <- ``dr.antialias``   (gradient to ``color``)
  * ``build_topology(tri)``   per-mesh host work (numpy): opposite vertices for the silhouette test and the CSR list
                              of each vertex's corners for the atomics-free attribute gradient
  * ``MeshRenderer``          ``Renderer.render`` for ``fix_geo: true`` / ``ssaa = 1``
  * ``projection`` / ``perspective``  the reference's camera matrices (numpy)

Two limits, both outside the reference's live configuration: there is no gradient with respect to vertex positions in
this module (``pos.requires_grad`` raises; moving geometry is ``mesh_deform``), and no near-plane clipping (a triangle with
a vertex at ``w <= 0`` is dropped).
Tensors follow nvdiffrast's shapes with the minibatch axis optional: ``pos`` [V,4] or [1,V,4], ``rast`` [H,W,4] or
[1,H,W,4], and so on; the output has a batch axis iff the image input had one.
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import _mesh_ops as ops
from ._launch import launch, require_gpu
from ._mesh_ops import MeshTopology, build_topology  # noqa: F401  (public names of this module too)

MAX_CHANNELS = 8
_POS_GRAD = ("gradients with respect to vertex positions are not implemented (nvdiffrast's rast_db and the position "
             "gradient of antialias): detach pos, or keep the geometry fixed (fix_geo: true)")


def rasterize(pos: torch.Tensor, tri: torch.Tensor, resolution) -> torch.Tensor:
    """``rast`` float32 [H,W,4] = (u, v, z/w, triangle id + 1), zeros where nothing is covered ([1,H,W,4] if ``pos`` is
    [1,V,4]).  ``pos``: float32 clip-space positions [V,4]; ``tri``: int32 [F,3]; ``resolution``: (H, W).  Row 0 is
    ``y_ndc = -1``.  Not differentiable."""
    require_gpu("rasterize", "pos", pos, torch.float32, 4)
    require_gpu("rasterize", "tri", tri, torch.int32, 3)
    if pos.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("rasterize: " + _POS_GRAD)
    p, batched = ops._unbatch("rasterize", "pos", pos.detach(), 2)
    if tri.dim() != 2:
        raise ValueError("rasterize: tri must be [F,3]")
    rast = ops.rasterize_forward(p.contiguous(), tri.contiguous(), int(resolution[0]), int(resolution[1]))
    return rast[None] if batched else rast


def interpolate(attr: torch.Tensor, rast: torch.Tensor, tri: torch.Tensor, pos: Optional[torch.Tensor] = None,
                topology: Optional[MeshTopology] = None) -> torch.Tensor:
    """``out`` [H,W,C] = (u a0 + v a1) + (1 - u - v) a2 of the covering triangle's corner attributes, 0 on background.
    ``attr``: float32 [V,C], C <= 8.  The gradient to ``attr`` walks each triangle's pixel box again and sums each
    vertex's corners in a fixed order (no atomics, bit-reproducible): it needs ``pos`` (what ``rast`` was made from) and
    uses ``topology`` (``build_topology(tri)`` if missing: a host pass over the mesh).  Without ``pos`` the op is
    forward-only and raises if ``attr`` requires a gradient."""
    require_gpu("interpolate", "attr", attr, torch.float32)
    require_gpu("interpolate", "rast", rast, torch.float32, 4)
    require_gpu("interpolate", "tri", tri, torch.int32, 3)
    a, b1 = ops._unbatch("interpolate", "attr", attr, 2)
    r, b2 = ops._unbatch("interpolate", "rast", rast.detach(), 3)
    if not 1 <= a.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"interpolate: attr must have 1..{MAX_CHANNELS} channels")
    p = None
    if pos is not None:
        require_gpu("interpolate", "pos", pos, torch.float32, 4)
        if pos.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("interpolate: " + _POS_GRAD)
        p = ops._unbatch("interpolate", "pos", pos.detach(), 2)[0].contiguous()
        if p.shape[0] != a.shape[0]:
            raise ValueError("interpolate: pos and attr must have one row per vertex")
    if a.requires_grad and torch.is_grad_enabled():
        if p is None:
            raise RuntimeError("interpolate: the gradient to attr walks each triangle's pixel box again and needs pos= "
                               "(the clip-space positions rast was made from)")
        if topology is None:
            topology = build_topology(tri, num_vertices=a.shape[0], device=a.device)
    if topology is not None:
        if not topology.corner_ptr.is_cuda or topology.corner_ptr.shape[0] != a.shape[0] + 1 \
                or topology.corner_idx.shape[0] != 3 * tri.shape[0]:
            raise ValueError("interpolate: topology does not belong to this mesh (or is not on the GPU)")
    out = ops._Interpolate.apply(a.contiguous(), r.contiguous(), tri.contiguous(), p, topology)
    return out[None] if (b1 or b2) else out


def antialias_weights(rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor, topology: MeshTopology) -> torch.Tensor:
    """``wts`` float32 [H,W,4]: the silhouette analysis of (rast, pos), shared by every image antialiased with them."""
    require_gpu("antialias", "rast", rast, torch.float32, 4)
    require_gpu("antialias", "pos", pos, torch.float32, 4)
    require_gpu("antialias", "tri", tri, torch.int32, 3)
    if pos.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("antialias: " + _POS_GRAD)
    r = ops._unbatch("antialias", "rast", rast.detach(), 3)[0].contiguous()
    p = ops._unbatch("antialias", "pos", pos.detach(), 2)[0].contiguous()
    t = tri.contiguous()
    if not topology.opp.is_cuda or tuple(topology.opp.shape) != tuple(t.shape):
        raise ValueError("antialias: topology does not belong to this mesh (or is not on the GPU)")
    H, W = r.shape[:2]
    wts = torch.empty((H, W, 4), dtype=torch.float32, device=r.device)
    launch("gd_mesh_antialias_weights", r.device, p.shape[0], t.shape[0], H, W, r, p, t, topology.opp.contiguous(), wts)
    return wts


def antialias(color: torch.Tensor, rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor,
              topology: Optional[MeshTopology] = None, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dr.antialias``: blends ``color`` [H,W,C] across silhouette edges.  The analysis depends on (rast, pos) only:
    pass ``weights=antialias_weights(...)`` to share it between images (``topology`` is then not needed); otherwise it
    is computed here from ``topology`` (``build_topology(tri)`` if that is missing too: a host pass over the mesh)."""
    require_gpu("antialias", "color", color, torch.float32)
    c, batched = ops._unbatch("antialias", "color", color, 3)
    if weights is None:
        if topology is None:
            topology = build_topology(tri, num_vertices=pos.shape[-2], device=color.device)
        weights = antialias_weights(rast, pos, tri, topology)
    else:
        require_gpu("antialias", "weights", weights, torch.float32, 4)
        if pos is not None and isinstance(pos, torch.Tensor) and pos.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("antialias: " + _POS_GRAD)
    if tuple(weights.shape) != (c.shape[0], c.shape[1], 4):
        raise ValueError("antialias: weights must be [H,W,4] of the colour's resolution")
    out = ops._Antialias.apply(c.contiguous(), weights.contiguous(), None, None, None, None)     # fixed geometry: no pos
    return out[None] if batched else out


def projection(fx, fy, cx, cy, width, height, n=0.01, f=1000):
    """``Renderer.projection`` (mesh_renderer.py:242-246): OpenGL projection from pinhole intrinsics, float32 [4,4]."""
    return np.array([[2.0 * fx / width, 0, 1.0 - 2.0 * cx / width, 0],
                     [0, 2.0 * fy / height, 1.0 - 2.0 * cy / height, 0],
                     [0, 0, -(f + n) / (f - n), -(2 * f * n) / (f - n)],
                     [0, 0, -1, 0.0]], dtype=np.float32)


def perspective(fovy, near=0.01, far=100):
    """``netf/view_core/camera.py:4-26``: ``fovy`` in radians, aspect 1, y flipped; float32 [4,4]."""
    y = np.tan(fovy / 2)
    return np.array([[1 / y, 0, 0, 0],
                     [0, -1 / y, 0, 0],
                     [0, 0, -(far + near) / (far - near), -(2 * far * near) / (far - near)],
                     [0, 0, -1, 0]], dtype=np.float32)


def safe_normalize(x: torch.Tensor, eps: float = 1e-20) -> torch.Tensor:
    """kiui.op.safe_normalize"""
    return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=eps))


class MeshRenderer:
    """``Renderer.render`` (mesh_renderer.py:338-428) for ``fix_geo: true``: a fixed mesh ``v`` [V,3] / ``f`` [F,3] with
    vertex normals ``vn`` [V,3], coloured by ``texture_fn``: any callable [N,3] -> [N,3] in [0,1] evaluated at the
    visible surface points (the reference's ``sigmoid(mlp(encoder(xyz)))``)."""

    def __init__(self, v: torch.Tensor, f: torch.Tensor, vn: torch.Tensor, texture_fn: Callable):
        require_gpu("MeshRenderer", "v", v, torch.float32, 3)
        require_gpu("MeshRenderer", "vn", vn, torch.float32, 3)
        require_gpu("MeshRenderer", "f", f)
        if v.requires_grad or vn.requires_grad:
            raise NotImplementedError("MeshRenderer: " + _POS_GRAD)
        self.v = v.detach().contiguous()
        self.f = f.detach().to(torch.int32).contiguous()
        self.vn = vn.detach().contiguous()
        self.texture_fn = texture_fn
        self.topology = build_topology(self.f, num_vertices=self.v.shape[0], device=self.v.device)

    def _matrices(self, pose, proj):
        """device float32 [4,4] each: inverse pose, projection, pose (``torch.inverse`` waits for the GPU)"""
        pose = torch.from_numpy(np.asarray(pose).astype(np.float32)).to(self.v.device)
        proj = torch.from_numpy(np.asarray(proj).astype(np.float32)).to(self.v.device)
        return torch.inverse(pose), proj, pose

    def _texture(self, xyzs, mask):
        """[N,3]: ``texture_fn`` at the points of ``xyzs`` [N,3] with ``mask`` (bool [N]), 0 elsewhere (waits for the GPU)"""
        color = torch.zeros_like(xyzs, dtype=torch.float32)
        if mask.any():
            color[mask] = self.texture_fn(xyzs[mask]).float()
        return color

    def _clip(self, mats):
        v_cam = torch.matmul(F.pad(self.v, pad=(0, 1), mode="constant", value=1.0), mats[0].T).float()
        return v_cam, (v_cam @ mats[1].T).contiguous()

    def clip_positions(self, pose, proj):
        """(v_cam [V,4], v_clip [V,4]) of the mesh under ``pose`` / ``proj`` (numpy [4,4]), as ``render`` forms them."""
        return self._clip(self._matrices(pose, proj))

    def render(self, pose, proj, h0, w0, ssaa=1, bg_color=1):
        """``pose`` (camera to world) and ``proj``: numpy [4,4].  Returns the reference's dict: ``image`` [H,W,3],
        ``alpha`` [H,W,1], ``depth`` [H,W,1], ``normal`` [H,W,3] in [0,1], ``cosinesview`` [H,W]."""
        if ssaa != 1:
            raise ValueError(f"{type(self).__name__}.render: ssaa != 1 is not implemented (the reference's trainer "
                             "passes 1)")
        h, w = int(h0), int(w0)
        v, f, topo = self.v, self.f, self.topology
        mats = self._matrices(pose, proj)
        v_cam, v_clip = self._clip(mats)

        rast = rasterize(v_clip, f, (h, w))
        wts = antialias_weights(rast, v_clip, f, topo)      # one analysis for alpha, colour, position and normal

        alpha = torch.clamp(rast[..., -1:], 0, 1).contiguous()
        alpha = antialias(alpha, rast, v_clip, f, weights=wts).clamp(0, 1)
        depth = interpolate(-v_cam[..., 2:3].contiguous(), rast, f)     # a slice: a list index would upload its indices
        xyzs_ = interpolate(v, rast, f)
        color = self._texture(xyzs_.view(-1, 3), (alpha > 0).view(-1)).view(h, w, 3)
        color = antialias(color, rast, v_clip, f, weights=wts).clamp(0, 1)
        color = alpha * color + (1 - alpha) * bg_color

        normal_ = interpolate(self.vn, rast, f)
        normal = safe_normalize(normal_)
        with torch.no_grad():
            position = antialias(xyzs_, rast, v_clip, f, weights=wts)
            normal_aa = antialias(normal_, rast, v_clip, f, weights=wts)
            view_direction = F.normalize(position - mats[2][:3, 3], dim=-1)
            cosines_view = F.cosine_similarity(view_direction, normal_aa, dim=-1, eps=1e-6)
        return {"image": color, "alpha": alpha, "depth": depth, "normal": (normal + 1) / 2, "cosinesview": cosines_view}
