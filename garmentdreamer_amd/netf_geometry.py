"""The NeTF stage with FREE geometry: the reference's ``Renderer`` for ``fix_geo: false``
(Garment_Deformer_NeTF/netf/render/mesh_renderer.py:129, 248-258, 315-335, 349-396), where the vertex offsets are trained
next to the hash grid and the MLP.  A composition of pieces that exist: the moving-geometry ops of ``mesh_deform``
(rasterize, interpolate, antialias with their gradients to the positions), the texture field's gradient to the sample
positions (``texture_field`` with ``position_gradient=True``; include/gd_texture_position.h), ``mesh_clean`` /
``mesh_remesh`` / ``mesh_simplify`` for ``remesh``, and ``gd_scene_adam_step`` for the optimizer -- no CPU path.

  * ``DeformableNeTFRenderer``   ``render`` differentiable in ``v_offsets`` and the field; ``remesh``; ``export_mesh`` and
                                 ``fit_texture_from_mesh`` through a ``NeTFRenderer`` on the current, detached geometry
  * ``DeformableNeTFOptimizer``  grid, MLP and offsets in one flat buffer, one launch per step
"""
from __future__ import annotations

import ctypes as C
from typing import Callable

import numpy as np
import torch
import torch.nn as nn

from . import mesh_deform as md
from ._launch import launch, require_gpu
from ._mesh_ops import build_topology
from .flat_adam import padded, reseat
from .mesh_render import antialias_weights, safe_normalize
from .texture_field import NeTFRenderer, TextureField


class DeformableNeTFRenderer(NeTFRenderer):
    """``Renderer`` with ``fix_geo: false``: the mesh is ``v = base_v + v_offsets`` / ``f``; ``base_v`` is fixed and
    ``v_offsets`` an ``nn.Parameter`` of zeros.  ``texture_fn(xyzs [H W,3], mask uint8 [H W])`` -> [H W,3] must accept
    points that require a gradient and pass one back: a ``TextureField`` with ``position_gradient=True``.

    ``render`` is ``NeTFRenderer.render`` on the current vertices, bit for bit at ``v_offsets == 0``, through the ops of
    ``mesh_deform``: ``image``, ``alpha`` and ``depth`` are differentiable in ``v_offsets`` (rasterize -> interpolate ->
    field -> antialias) and in the field's parameters.  The vertex normals are recomputed on every render from the current
    ``v`` by the reference's formula for this mode (the SUM of the unit face normals, not normalised; (0, 0, 1) where its
    squared length is <= 1e-20), each vertex's faces gathered in ``topology.corner_idx`` order, no float atomics.
    ``normal`` and ``cosinesview`` carry NO gradient to the geometry: no loss of the reference's trainer reads them
    (trainer.py:189-216 uses ``image`` only).  Nothing in a render, its backward and an optimizer step waits for the GPU.
    """

    def __init__(self, v: torch.Tensor, f: torch.Tensor, texture_fn: Callable):
        require_gpu("DeformableNeTFRenderer", "v", v, torch.float32, 3)
        require_gpu("DeformableNeTFRenderer", "f", f)
        if isinstance(texture_fn, TextureField) and not texture_fn.encoder.position_gradient:
            raise ValueError("DeformableNeTFRenderer: the field must pass a gradient to its sample positions: "
                             "TextureField(..., position_gradient=True)")
        self.texture_fn = texture_fn
        self._set_mesh(v, f)

    def _set_mesh(self, v, f):
        self.base_v = v.detach().contiguous().clone()
        self.f = f.detach().to(torch.int32).contiguous()
        self.v_offsets = nn.Parameter(torch.zeros_like(self.base_v))
        self.topology = build_topology(self.f, num_vertices=self.base_v.shape[0], device=self.base_v.device)
        # [V, K] faces around each vertex in corner_idx order, K the largest count; the padding names row F (zeros)
        ptr = self.topology.corner_ptr.cpu().numpy().astype(np.int64)
        faces = self.topology.corner_idx.cpu().numpy().astype(np.int64) // 3
        count = np.diff(ptr)
        table = np.full((count.shape[0], max(int(count.max()) if count.size else 0, 1)), self.f.shape[0], dtype=np.int64)
        rows = np.repeat(np.arange(count.shape[0]), count)
        table[rows, np.arange(faces.shape[0]) - ptr[rows]] = faces
        self._vertex_faces = torch.from_numpy(table).to(self.base_v.device)
        self._up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float32, device=self.base_v.device)

    @property
    def v(self) -> torch.Tensor:
        return self.base_v + self.v_offsets

    @property
    def vn(self) -> torch.Tensor:
        """the current vertex normals (what ``render`` interpolates), detached"""
        return self.vertex_normals()

    @torch.no_grad()
    def vertex_normals(self) -> torch.Tensor:
        """[V,3] of the current ``v``: mesh_renderer.py:385-396, the scatter_add as a gather in a fixed order"""
        v, f = self.v, self.f.long()
        v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        fn = safe_normalize(torch.cross(v1 - v0, v2 - v0, dim=-1))
        fn = torch.cat([fn, fn.new_zeros(1, 3)])
        vn = fn[self._vertex_faces].sum(dim=1)
        return torch.where(torch.sum(vn * vn, -1, keepdim=True) > 1e-20, vn, self._up)

    def frozen(self) -> NeTFRenderer:
        """a ``NeTFRenderer`` on the current vertices and normals, detached (the same ``f`` and ``texture_fn``)"""
        return NeTFRenderer(self.v.detach(), self.f, self.vertex_normals(), self.texture_fn)

    def _clip_of(self, v, mats):
        v_cam = torch.matmul(torch.nn.functional.pad(v, pad=(0, 1), mode="constant", value=1.0), mats[0].T).float()
        return v_cam, (v_cam @ mats[1].T).contiguous()

    def _clip(self, mats):
        return self._clip_of(self.v.detach(), mats)

    def render(self, pose, proj, h0, w0, ssaa=1, bg_color=1):
        """``pose`` (camera to world) and ``proj``: numpy [4,4].  Returns the reference's dict: ``image`` [H,W,3],
        ``alpha`` [H,W,1], ``depth`` [H,W,1], ``normal`` [H,W,3] in [0,1], ``cosinesview`` [H,W]."""
        if ssaa != 1:
            raise ValueError(f"{type(self).__name__}.render: ssaa != 1 is not implemented (the reference's trainer "
                             "passes 1)")
        h, w = int(h0), int(w0)
        v, f, topo = self.v, self.f, self.topology
        mats = self._matrices(pose, proj)
        v_cam, v_clip = self._clip_of(v, mats)

        rast = md.rasterize(v_clip, f, (h, w), topo)
        wts = antialias_weights(rast.detach(), v_clip.detach(), f, topo)    # one analysis for every image of this view

        alpha = torch.clamp(rast[..., -1:], 0, 1).contiguous()
        alpha = md.antialias(alpha, rast, v_clip, f, topo, weights=wts).clamp(0, 1)
        depth = md.interpolate(-v_cam[..., 2:3].contiguous(), rast, f, v_clip, topo)
        xyzs_ = md.interpolate(v, rast, f, v_clip, topo)
        color = self._texture(xyzs_.view(-1, 3), (alpha > 0).view(-1)).view(h, w, 3)
        color = md.antialias(color, rast, v_clip, f, topo, weights=wts).clamp(0, 1)
        color = alpha * color + (1 - alpha) * bg_color

        with torch.no_grad():
            normal_ = md.interpolate(self.vertex_normals(), rast, f, v_clip, topo)
            normal = safe_normalize(normal_)
            position = md.antialias(xyzs_, rast, v_clip, f, topo, weights=wts)
            normal_aa = md.antialias(normal_, rast, v_clip, f, topo, weights=wts)
            view_direction = torch.nn.functional.normalize(position - mats[2][:3, 3], dim=-1)
            cosines_view = torch.nn.functional.cosine_similarity(view_direction, normal_aa, dim=-1, eps=1e-6)
        return {"image": color, "alpha": alpha, "depth": depth, "normal": (normal + 1) / 2, "cosinesview": cosines_view}

    def get_params(self, hashgrid_lr=0.01, mlp_lr=0.001, geom_lr=0.0001):
        """The reference's three groups (mesh_renderer.py:248-258); ``texture_fn`` must be a ``TextureField``."""
        return self._field("get_params").get_params(hashgrid_lr, mlp_lr) + [{"params": [self.v_offsets], "lr": geom_lr}]

    def optimizer(self, hashgrid_lr=0.01, mlp_lr=0.001, geom_lr=0.0001, betas=(0.9, 0.999),
                  eps=1e-8) -> "DeformableNeTFOptimizer":
        """Adam over the three groups as one launch per step.  It holds THIS ``v_offsets``: build a new one after
        ``remesh``."""
        return DeformableNeTFOptimizer(self, hashgrid_lr, mlp_lr, geom_lr, betas, eps)

    def _field(self, what) -> TextureField:
        if not isinstance(self.texture_fn, TextureField):
            raise TypeError(f"DeformableNeTFRenderer.{what}: texture_fn must be a TextureField")
        return self.texture_fn

    @torch.no_grad()
    def remesh(self, remesh_size=0.015, decimate_target=50000, remesh_iters=3) -> dict:
        """``Renderer.remesh`` (mesh_renderer.py:326-335) on the current vertices: ``clean_mesh(repair=False)`` with its
        defaults (they mirror kiui's), ``remesh_botsch(h=remesh_size, iterations=remesh_iters)``, then
        ``decimate_quadric(decimate_target)`` if more than ``decimate_target > 0`` faces are left.  If the remesher refuses
        the cleaned mesh as non-manifold, it is cleaned again with ``repair=True`` (``report["repaired"]``).  Then ``base_v``
        and ``f`` are replaced, ``v_offsets`` is a NEW zero parameter, topology and normals are rebuilt -- and an optimizer
        built before holds the old parameter: build a new one.  (In the reference the new parameter silently falls out of
        the trainer's optimizer; that is documented here, not copied.)  kiui is not installed next to this project: the
        iteration count of its remesher (``remesh_iters``) and its agreement with ``remesh_botsch`` are unverified.
        Waits for the GPU (host passes of the three operations).  Returns a report: the three operations' own reports
        and the sizes before and after."""
        from . import mesh_clean, mesh_remesh, mesh_simplify
        v, f = self.v.detach().contiguous(), self.f
        report = {"vertices_before": int(v.shape[0]), "faces_before": int(f.shape[0]), "repaired": False}
        cleaned = mesh_clean.clean_mesh(v, f, repair=False)
        try:
            v2, f2, info = mesh_remesh.remesh_botsch(cleaned.vertices, cleaned.indices, h=remesh_size,
                                                     iterations=remesh_iters)
        except ValueError as e:
            if "non-manifold" not in str(e):
                raise
            cleaned = mesh_clean.clean_mesh(v, f, repair=True)
            report["repaired"] = True
            v2, f2, info = mesh_remesh.remesh_botsch(cleaned.vertices, cleaned.indices, h=remesh_size,
                                                     iterations=remesh_iters)
        report["clean"], report["remesh"] = cleaned.report, info
        if decimate_target > 0 and f2.shape[0] > decimate_target:
            v2, f2, report["decimate"] = mesh_simplify.decimate_quadric(v2, f2, decimate_target)
        if f2.shape[0] == 0:
            raise ValueError("DeformableNeTFRenderer.remesh: no face of the mesh is left")
        self._set_mesh(v2, f2)
        report["vertices_after"], report["faces_after"] = int(v2.shape[0]), int(f2.shape[0])
        return report

    def fit_texture_from_mesh(self, views, iters=600, resolution=1024, hashgrid_lr=0.01, mlp_lr=0.001, seed=0,
                              save_path=None, optimizer=None):
        """``NeTFRenderer.fit_texture_from_mesh`` on the current geometry, detached: only the field is fitted."""
        return self.frozen().fit_texture_from_mesh(views, iters, resolution, hashgrid_lr, mlp_lr, seed, save_path,
                                                   optimizer)

    def export_mesh(self, save_path, texture_resolution=2048, padding=16, reverse=False, vt=None, ft=None, atlas="grid"):
        """``NeTFRenderer.export_mesh`` of the current ``v.detach()``: the moved vertices are what is baked and written."""
        return self.frozen().export_mesh(save_path, texture_resolution, padding, reverse, vt, ft, atlas)


class DeformableNeTFOptimizer:
    """``torch.optim.Adam(renderer.get_params(...))`` as ONE ``gd_scene_adam_step`` launch over one flat buffer holding the
    grid, then the MLP, then the vertex offsets, the three ranges with their own learning rate; ``zero_grad`` is ONE memset.
    ``TextureFieldOptimizer`` with a third range: the parameters are re-seated NOW as views of the flat buffer and their
    ``.grad`` are, for good, views of the flat gradient buffer (the field's backward adds straight into it; autograd
    accumulates the offsets' gradient into its view in place).  A parameter always has a gradient here, so its moments
    decay on every step."""

    def __init__(self, renderer: DeformableNeTFRenderer, hashgrid_lr=0.01, mlp_lr=0.001, geom_lr=0.0001, betas=(0.9, 0.999),
                 eps=1e-8):
        field_module = renderer._field("optimizer")
        grid = [field_module.encoder.params]
        mlp = list(field_module.mlp.parameters())
        geom = [renderer.v_offsets]
        for p in grid + mlp + geom:
            require_gpu("DeformableNeTFOptimizer", "every parameter", p, torch.float32)
        self._flat, self._grad, self._exp_avg, self._exp_avg_sq, _ = reseat(grid + mlp + geom)
        mlp_end = padded(grid[0].numel()) + sum(padded(p.numel()) for p in mlp)
        self._ends = (C.c_int64 * 3)(padded(grid[0].numel()), mlp_end, self._flat.numel())
        self.param_groups = [{"params": grid, "lr": float(hashgrid_lr)}, {"params": mlp, "lr": float(mlp_lr)},
                             {"params": geom, "lr": float(geom_lr)}]
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.step_count = 0

    def zero_grad(self, set_to_none: bool = False):
        self._grad.zero_()

    @torch.no_grad()
    def step(self):
        self.step_count += 1
        lrs = (C.c_double * 3)(*[float(g["lr"]) for g in self.param_groups])
        launch("gd_scene_adam_step", self._flat.device, self._flat, self._grad, self._exp_avg, self._exp_avg_sq,
               self._flat.numel(), 3, self._ends, lrs, self.betas[0], self.betas[1], self.eps, self.step_count)
