"""One iteration of the mesh deformer's first stage (stage 3 of the reference, ``Garment_Deformer_NeTF/deformation.py``:
the loop over ``progress_bar_first``): Adam on vertex offsets under a mask loss, the normal-consistency loss and the
uniform Laplacian loss, on the HIP kernels of ``mesh_deform`` (render) and ``mesh_geometry`` (normals and the two geometry
losses) -- no CPU path.

Out of scope here: the second stage's other losses (``normal``, ``hole_mask``, ``shading`` and its neural shader),
remeshing, reading the views, the space normalisation and the image dumps.  The second stage's update RULE is built
(``step(..., only_visible=True)``), so a caller can add its own losses on top of it.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import mesh_geometry as mg
from ._launch import require_gpu
from .flat_adam import FlatAdam
from .mesh_deform import GBufferRenderer

FIRST_STAGE_WEIGHTS = {"mask": 2, "normal_consistency": 0.1, "laplacian": 800}   # deformation.py, loss_weights_first
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
            with torch.no_grad():
                visible = self.renderer.vertex_visibility(mvps, vertices.detach(), geo.tri, resolutions)
                g = self.offsets.grad
                stepped = self.offsets - self.lr * g / (g.abs() + self.eps)
                self.offsets.copy_(torch.where(visible[:, None], stepped, self.offsets))
        else:
            self.optimizer.step()
        out = {k: v.detach() for k, v in losses.items()}
        out["total"] = total.detach()
        return out
