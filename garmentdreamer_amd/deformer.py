"""Iterations of the mesh deformer (stage 3 of the reference, ``Garment_Deformer_NeTF/deformation.py``).

First stage (the loop over ``progress_bar_first``, ``Deformer.step``): Adam on vertex offsets under a mask loss, the
normal-consistency loss and the uniform Laplacian loss, on the HIP kernels of ``mesh_deform`` (render) and ``mesh_geometry``
(normals and the two geometry losses).

Second stage (the loop over ``progress_bar_second``, ``begin_second_stage`` / ``step_second`` / ``remesh``): the same
three terms plus the normal-map loss and the hole-mask loss against a frozen copy of the mesh, on the kernels of
``mesh_losses``, under the visible-rows update ``lr g / (|g| + eps)``; with a ``neural_shader.NeuralShader`` also the
``shading`` loss (``mesh_losses.shading_loss``) and the shader's own Adam; at an upsample iteration ``remesh`` remeshes
the current mesh on the kernels of ``mesh_remesh`` and ``adopt_remesh`` carries on from the result.  ``final_mesh`` is the
stage's product: the current mesh rotated upright, decimated and smoothed on the kernels of ``mesh_simplify``.  No CPU path
anywhere.

From disk: ``Deformer.from_views`` / ``begin_second_stage_from_views`` take the views of ``views.read_views``, and
``run_deformation`` is the whole schedule of ``deformation.py`` on a capture directory: read, adjust, normalise, both stages
with the upsample, denormalise, post-process, write.

Out of scope here: the image dumps and the parsing of the YAML configuration.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch

from . import mesh_geometry as mg
from . import mesh_losses as ml
from . import mesh_remesh as mr
from . import mesh_simplify as ms
from . import template
from . import views as gv
from ._launch import require_gpu
from .flat_adam import FlatAdam
from .mesh_deform import GBufferRenderer
from .neural_shader import NeuralShader

FIRST_STAGE_WEIGHTS = {"mask": 2, "normal_consistency": 0.1, "laplacian": 800}   # deformation.py, loss_weights_first
# deformation.py, loss_weights_second with the defaults of its arguments; its "shading": 1.0 is begin_second_stage's
# shading_weight, applied when a shader is given
SECOND_STAGE_WEIGHTS = {"hole_mask": 2.0, "mask": 2.0, "normal_consistency": 0.1, "laplacian": 40.0, "normal": 0.8}
CHANNELS = ["mask", "position", "normal"]


class Deformer:
    """``vertices`` float32 [V,3] and ``indices`` [F,3] on the GPU: the initial mesh.  ``mvps``: one ``to_gl_camera`` matrix
    [4,4] per view, ``target_masks``: one mask [H,W,1] per view, ``resolutions``: (H, W) per view or one for all, all on the
    GPU already (``step`` copies nothing from the host).  The optimised quantity is ``offsets`` [V,3], zero at the start;
    the mesh of an iteration is ``initial + offsets``."""

    def __init__(self, vertices: torch.Tensor, indices: torch.Tensor, mvps, target_masks: Sequence[torch.Tensor],
                 resolutions, lr: float = 1e-3, weights: Optional[Dict[str, float]] = None):
        require_gpu("Deformer", "vertices", vertices, torch.float32, 3)
        require_gpu("Deformer", "indices", indices)
        dev = vertices.device
        self.initial = vertices.detach().clone().contiguous()
        self.geometry = mg.build_geometry(indices, num_vertices=vertices.shape[0], device=dev)
        self.renderer = GBufferRenderer()
        mvps, self.resolutions = GBufferRenderer._views(mvps, resolutions)
        self.mvps = [torch.as_tensor(m, dtype=torch.float32).to(dev) for m in mvps]
        self.target_masks = [require_gpu("Deformer", "target mask", m, torch.float32, 1) for m in target_masks]
        if len(self.target_masks) != len(self.mvps):
            raise ValueError("Deformer: one target mask per view")
        self.weights = dict(FIRST_STAGE_WEIGHTS if weights is None else weights)
        self.offsets = torch.nn.Parameter(torch.zeros_like(self.initial))
        self.optimizer = FlatAdam([self.offsets], lr=lr)
        self.eps = self.optimizer.eps

    @classmethod
    def from_views(cls, vertices: torch.Tensor, indices: torch.Tensor, views, near: float, far: float, **kw) -> "Deformer":
        """The constructor fed from ``views.read_views``: one ``to_gl_camera`` matrix per view between ``near`` and ``far``
        (``views.near_far``), its mask as the target and its resolution; ``kw`` goes to the constructor."""
        return cls(vertices, indices, gv.view_mvps(views, near, far), [v.mask for v in views],
                   [v.resolution for v in views], **kw)

    @property
    def lr(self) -> float:
        return self.optimizer.lr

    def step(self, view_indices: Sequence[int], only_visible: bool = False) -> Dict[str, torch.Tensor]:
        """One iteration on the views ``view_indices``: deform, normals, render mask / position / normal with
        antialiasing, the three weighted losses, backward, update.  Returns the detached losses (``mask``,
        ``normal_consistency``, ``laplacian``, ``total``) as device tensors; nothing in here waits for the GPU.

        ``only_visible=False`` is the first stage: one step of the Adam that lives as long as this object.

        ``only_visible=True`` is the second stage's rule.  There the reference builds, on EVERY iteration, a fresh
        ``torch.optim.Adam`` over a copy of the visible vertices' offsets, steps it once and writes the result back; the
        other offsets are carried over untouched.  The first step of Adam from zero moments with gradient g is
        m = (1 - b1) g, v = (1 - b2) g^2, the bias corrections divide them by exactly (1 - b1) and (1 - b2), so
        m_hat = g, v_hat = g^2, and the update is  lr m_hat / (sqrt(v_hat) + eps) = lr g / (|g| + eps):  b1, b2 and any
        history drop out.  That is what is applied here, to the rows of ``GBufferRenderer.vertex_visibility`` for these
        views (8x upsampled, as the reference); the moments of the first stage's Adam are neither read nor written."""
        views = [int(i) for i in view_indices]
        mvps = [self.mvps[i] for i in views]
        resolutions = [self.resolutions[i] for i in views]
        geo = self.geometry
        self.offsets.grad = None
        vertices = self.initial + self.offsets
        face_normals, vertex_normals = mg.normals(vertices, geo)
        gbuffers = self.renderer.render(mvps, vertices, geo.tri, vertex_normals, resolutions, CHANNELS,
                                        with_antialiasing=True, topology=geo.topology)
        losses = {"mask": mg.mask_loss([self.target_masks[i] for i in views], gbuffers),
                  "normal_consistency": mg.normal_consistency_loss(face_normals, geo),
                  "laplacian": mg.laplacian_loss(vertices, geo)}
        total = sum(losses[k] * float(w) for k, w in self.weights.items() if w > 0)
        total.backward()
        if only_visible:
            self._step_visible(mvps, vertices, resolutions)
        else:
            self.optimizer.step()
        out = {k: v.detach() for k, v in losses.items()}
        out["total"] = total.detach()
        return out

    def _step_visible(self, mvps, vertices: torch.Tensor, resolutions) -> None:
        """The second stage's update (see ``step``): ``lr g / (|g| + eps)`` on the rows visible in these views."""
        with torch.no_grad():
            visible = self.renderer.vertex_visibility(mvps, vertices.detach(), self.geometry.tri, resolutions)
            g = self.offsets.grad
            stepped = self.offsets - self.lr * g / (g.abs() + self.eps)
            self.offsets.copy_(torch.where(visible[:, None], stepped, self.offsets))

    # ---- second stage ------------------------------------------------------------------------------------------------

    def begin_second_stage(self, target_normals: Sequence[torch.Tensor], camera_Rs, camera_centers,
                           weights: Optional[Dict[str, float]] = None, enhanced: bool = True,
                           target_rgbs: Optional[Sequence[torch.Tensor]] = None, shader=None,
                           shading_percentage: float = 0.75, shading_weight: float = 1.0, lr_shader: float = 1e-3,
                           seed: int = 0) -> None:
        """Enter the second stage (deformation.py:264-267).  ``target_normals``: one estimated normal map [H,W,3] in [0,1]
        per view, in the camera's frame; ``camera_Rs`` [3,3] and ``camera_centers`` [3]: each view's rotation and centre,
        all on the GPU.  ``weights``: ``SECOND_STAGE_WEIGHTS`` by default; ``enhanced`` selects
        ``normal_map_loss_enhanced`` (the reference's default) or ``normal_map_loss`` for the ``normal`` term.  The mesh of
        this moment, ``initial + offsets``, is frozen with its normals as the reference mesh of the hole-mask loss.

        ``shader``: a ``neural_shader.NeuralShader``; with one, ``target_rgbs`` (one image [H,W,3] per view) is required and
        ``step_second`` adds ``shading_weight`` x ``shading_loss`` over ``shading_percentage`` of the valid pixels, sampled by
        ``seed`` and the iteration counter, and steps the shader's Adam (``lr_shader``) next to the vertex update."""
        n = len(self.mvps)
        if len(target_normals) != n or len(camera_Rs) != n or len(camera_centers) != n:
            raise ValueError("Deformer: one normal map, one rotation and one centre per view")
        if shader is not None and (target_rgbs is None or len(target_rgbs) != n):
            raise ValueError("Deformer: a shader needs one target image per view")
        rgbs = [None] * n if shader is None else [require_gpu("Deformer", "target rgb", t, torch.float32, 3) for t in target_rgbs]
        self.views = [ml.View(require_gpu("Deformer", "target normal", t, torch.float32, 3), m,
                              require_gpu("Deformer", "camera R", R, torch.float32),
                              require_gpu("Deformer", "camera centre", c, torch.float32), rgb)
                      for t, m, R, c, rgb in zip(target_normals, self.target_masks, camera_Rs, camera_centers, rgbs)]
        self.shader = shader
        self.shader_optimizer = None if shader is None else shader.optimizer(lr=lr_shader)
        self.shading_percentage, self.shading_weight = float(shading_percentage), float(shading_weight)
        self.shading_seed, self.second_iteration = int(seed), 0
        self.cameras = [ml.camera_block(view) for view in self.views]
        self.second_weights = dict(SECOND_STAGE_WEIGHTS if weights is None else weights)
        self.enhanced = bool(enhanced)
        with torch.no_grad():
            self.rf_geometry = self.geometry
            self.rf_vertices = (self.initial + self.offsets).detach().clone()
            self.rf_normals = mg.normals(self.rf_vertices, self.rf_geometry)[1]

    def begin_second_stage_from_views(self, views, **kw) -> None:
        """``begin_second_stage`` with the normal maps, rotations, centres and colour images of ``views`` (the list this
        object was made from by ``from_views``); ``kw`` carries its other arguments."""
        dev = self.initial.device
        self.begin_second_stage([v.normal for v in views], [v.R.to(dev) for v in views], [v.center.to(dev) for v in views],
                                target_rgbs=[v.rgb for v in views], **kw)

    def step_second(self, view_indices: Sequence[int],
                    extra_loss: Optional[Callable[[Sequence[int], Sequence[dict]], torch.Tensor]] = None
                    ) -> Dict[str, torch.Tensor]:
        """One second-stage iteration on the views ``view_indices`` (deformation.py:297-355): deform, normals, render the
        mesh with gradients and the frozen reference mesh without, the five weighted losses (``mask``,
        ``normal_consistency``, ``laplacian``, ``normal``, ``hole_mask``; the last two from one fused call per view),
        with a shader the weighted ``shading`` term, backward, the visible-rows update of ``step(only_visible=True)`` and
        the shader's Adam step.  ``extra_loss(view_indices, gbuffers)``: a term the caller adds, already weighted; it is
        returned as ``extra``.  Returns the detached losses as device tensors; nothing in here waits for the GPU."""
        if not hasattr(self, "views"):
            raise RuntimeError("Deformer.step_second: call begin_second_stage first")
        views = [int(i) for i in view_indices]
        mvps = [self.mvps[i] for i in views]
        resolutions = [self.resolutions[i] for i in views]
        geo, rf = self.geometry, self.rf_geometry
        self.offsets.grad = None
        vertices = self.initial + self.offsets
        face_normals, vertex_normals = mg.normals(vertices, geo)
        gbuffers = self.renderer.render(mvps, vertices, geo.tri, vertex_normals, resolutions, CHANNELS,
                                        with_antialiasing=True, topology=geo.topology)
        with torch.no_grad():
            gbuffers_rf = self.renderer.render(mvps, self.rf_vertices, rf.tri, self.rf_normals, resolutions, CHANNELS,
                                               with_antialiasing=True, topology=rf.topology)
        fused = ml.second_stage_losses([self.views[i] for i in views], gbuffers, gbuffers_rf, self.enhanced,
                                       cameras=[self.cameras[i] for i in views])
        losses = {"mask": mg.mask_loss([self.target_masks[i] for i in views], gbuffers),
                  "normal_consistency": mg.normal_consistency_loss(face_normals, geo),
                  "laplacian": mg.laplacian_loss(vertices, geo),
                  "normal": fused["normal"], "hole_mask": fused["hole_mask"]}
        total = sum(losses[k] * float(w) for k, w in self.second_weights.items() if w > 0)
        if self.shader is not None:
            self.shader_optimizer.zero_grad()
            losses["shading"] = ml.shading_loss([self.views[i] for i in views], gbuffers, self.shader,
                                                self.shading_percentage, self.shading_seed, self.second_iteration)
            total = total + losses["shading"] * self.shading_weight
            self.second_iteration += 1
        if extra_loss is not None:
            losses["extra"] = extra_loss(views, gbuffers)
            total = total + losses["extra"]
        total.backward()
        self._step_visible(mvps, vertices, resolutions)
        if self.shader is not None:
            self.shader_optimizer.step()
        out = {k: v.detach() for k, v in losses.items()}
        out["total"] = total.detach()
        return out

    def remesh(self, h: Optional[float] = None) -> Dict[str, list]:
        """An upsample iteration (deformation.py:273-295): remesh the current mesh ``initial + offsets`` towards edge
        length ``h`` (default: half its mean edge length, as the reference) with ``mesh_remesh.remesh_botsch`` and continue
        on the result through ``adopt_remesh``.  Returns the remesher's ``info``.  Reads counts back from the GPU."""
        if not hasattr(self, "views"):
            raise RuntimeError("Deformer.remesh: call begin_second_stage first")
        vertices = (self.initial + self.offsets).detach()
        if h is None:
            h = 0.5 * float(mr.mean_edge_length(vertices, self.geometry))
        new_vertices, new_indices, info = mr.remesh_botsch(vertices, self.geometry.tri, h)
        self.adopt_remesh(new_vertices, new_indices)
        return info

    def final_mesh(self, target_faces: int = 40000, smooth: bool = True, rotate: bool = True):
        """The mesh the stage hands on (``write_mesh(..., 'final_mesh.obj', final_mesh, post_process=True)``,
        deformation.py's last line): ``mesh_simplify.post_process_mesh`` of the current mesh ``initial + offsets``, as
        ``(vertices float32 [V',3], indices int32 [F',3])`` for ``mesh_simplify.write_obj``.  Nothing of this object
        changes.  Reads counts back from the GPU."""
        vertices = (self.initial + self.offsets).detach()
        new_vertices, new_indices, _ = ms.post_process_mesh(vertices, self.geometry.tri, target_faces, smooth, rotate)
        return new_vertices, new_indices

    def adopt_remesh(self, vertices: torch.Tensor, indices: torch.Tensor) -> None:
        """Continue the second stage on a remeshed surface (deformation.py:273-295; the remeshing itself is the caller's):
        ``vertices`` / ``indices`` become the initial mesh with zero offsets, the ``laplacian`` and ``normal_consistency``
        weights are multiplied by 4 and ``lr`` by 0.25.  The frozen reference mesh keeps its own geometry."""
        if not hasattr(self, "views"):
            raise RuntimeError("Deformer.adopt_remesh: call begin_second_stage first")
        require_gpu("Deformer", "vertices", vertices, torch.float32, 3)
        require_gpu("Deformer", "indices", indices)
        self.initial = vertices.detach().clone().contiguous()
        self.geometry = mg.build_geometry(indices, num_vertices=vertices.shape[0], device=vertices.device)
        for k in ("laplacian", "normal_consistency"):
            if k in self.second_weights:
                self.second_weights[k] *= 4
        self.offsets = torch.nn.Parameter(torch.zeros_like(self.initial))
        self.optimizer = FlatAdam([self.offsets], lr=self.lr * 0.25)


# ---- the whole stage --------------------------------------------------------------------------------------------------

# configs/garment_deformer_configs.yml of the reference, the keys this schedule reads; ``final_faces`` is the target of
# write_mesh(..., post_process=True)
DEFAULT_CONFIG = {
    "enhanced_normal_map_loss": True, "iterations_first": 3000, "iterations_second": 1000, "upsample_iterations": [3500],
    "lr_vertices": 0.001, "weight_hole_mask": 2.0, "weight_mask": 2.0, "weight_normal_consistency": 0.1,
    "weight_laplacian": 40.0, "weight_normal": 0.8, "weight_shading": 1.0, "lr_shader": 0.001, "shading_percentage": 0.75,
    "hidden_features_layers": 3, "hidden_features_size": 256, "fourier_features": "positional", "activation": "relu",
    "fft_scale": 4, "picked_views_first": [74, 333],
    "picked_views_second": [111, 115, 120, 125, 129, 133, 138, 143, 221, 189, 194, 199, 203, 207, 212, 217,
                            259, 263, 268, 273, 277, 281, 286, 291],
    "final_faces": 40000,
}


def run_deformation(directory: str, template_obj: str, bound: float, config: Optional[dict] = None) -> Dict[str, str]:
    """The schedule of ``deformation.py`` on the capture in ``directory`` (``views.read_views``'s layout) from the template
    mesh ``template_obj``, without the image dumps: the seeds; the template adjusted by ``bound``, its box saved, views,
    mesh and box normalised, near and far over ALL cameras; the first stage over the views at positions
    ``picked_views_first[0] .. [1]``, one drawn per iteration; the second stage over ``picked_views_second`` under the
    visible-rows rule, with ``remesh`` at an upsample iteration; the mesh denormalised, written, post-processed and written
    again.  ``config``: overrides of ``DEFAULT_CONFIG`` (a dict; YAML is the caller's).  Only the views either stage can
    draw are read.  Returns the paths written: ``bbox``, ``mesh`` and ``final_mesh``."""
    unknown = set(config or {}) - set(DEFAULT_CONFIG)
    if unknown:
        raise ValueError(f"run_deformation: unknown config keys {sorted(unknown)}")
    cfg = {**DEFAULT_CONFIG, **(config or {})}
    np.random.seed(12)
    torch.manual_seed(123)
    torch.cuda.manual_seed(123)
    directory = os.fspath(directory)
    out_dir = os.path.join(directory, "deformation_check")
    os.makedirs(os.path.join(out_dir, "meshes"), exist_ok=True)

    cameras = gv.read_cameras(directory)
    first = [i for i in range(*cfg["picked_views_first"]) if i < len(cameras)]
    second = sorted(set(int(i) for i in cfg["picked_views_second"] if 0 <= int(i) < len(cameras)))
    wanted = sorted(set(first) | set(second))
    views = gv.read_views(directory, indices=wanted)
    place = {p: k for k, p in enumerate(wanted)}                       # position in the capture -> position in `views`

    v, f = template.load_obj(template_obj)
    vertices = gv.adjust_template(v, bound).astype(np.float32)
    aabb = gv.AABB(vertices)
    paths = {"bbox": os.path.join(out_dir, "bbox.txt")}
    aabb.save(paths["bbox"])
    space = gv.SpaceNormalization(aabb.corners)
    space.normalize_views(views)
    space.normalize_views(cameras)
    vertices = space.normalize_mesh(vertices).astype(np.float32)
    near, far = gv.near_far(cameras, space.normalize_aabb(aabb).corners, epsilon=0.5)

    dev = views[0].mask.device
    deformer = Deformer.from_views(torch.from_numpy(vertices).to(dev), torch.from_numpy(f.astype(np.int32)).to(dev), views,
                                   near, far, lr=cfg["lr_vertices"])
    sampler_first = gv.ViewSampler(views, "several", 1, [place[i] for i in first])
    sampler_second = gv.ViewSampler(views, "several", 1, [place[i] for i in second])
    for _ in range(int(cfg["iterations_first"])):
        deformer.step(sampler_first())

    shader = None
    if cfg["weight_shading"] > 0:
        shader = NeuralShader(hidden_features_size=cfg["hidden_features_size"],
                              hidden_features_layers=cfg["hidden_features_layers"], activation=cfg["activation"],
                              fourier_features=cfg["fourier_features"], fft_scale=cfg["fft_scale"], device=dev)
    weights = {"hole_mask": cfg["weight_hole_mask"], "mask": cfg["weight_mask"],
               "normal_consistency": cfg["weight_normal_consistency"], "laplacian": cfg["weight_laplacian"],
               "normal": cfg["weight_normal"]}
    deformer.begin_second_stage_from_views(views, weights=weights, enhanced=bool(cfg["enhanced_normal_map_loss"]),
                                           shader=shader, shading_percentage=cfg["shading_percentage"],
                                           shading_weight=cfg["weight_shading"], lr_shader=cfg["lr_shader"])
    start, total = int(cfg["iterations_first"]) + 1, int(cfg["iterations_first"]) + int(cfg["iterations_second"])
    for iteration in range(start, total + 1):
        if iteration in cfg["upsample_iterations"]:
            deformer.remesh()
        deformer.step_second(sampler_second())

    final = space.denormalize_mesh((deformer.initial + deformer.offsets).detach())
    paths["mesh"] = os.path.join(out_dir, "meshes", f"mesh_{total:06d}.obj")
    ms.write_obj(paths["mesh"], final, deformer.geometry.tri)
    processed, processed_tri, _ = ms.post_process_mesh(final.contiguous(), deformer.geometry.tri, int(cfg["final_faces"]))
    paths["final_mesh"] = os.path.join(directory, "final_mesh.obj")
    ms.write_obj(paths["final_mesh"], processed, processed_tri)
    return paths
