"""The first half of the NeTF stage: fitting the texture field to the captured views
(``Renderer.fit_texture_from_mesh``, Garment_Deformer_NeTF/netf/render/mesh_renderer.py:158-240), with the tail of the
render and the masked MSE fused into the HIP loss head of ``csrc/raster_fit.hip`` (C-ABI and definitions: include/gd_fit.h)
-- no CPU path.

  * ``fit_pose(c2w)``                       the reference's camera of a captured view (host numpy)
  * ``fit_projection(K, width, height)``    ``mesh_render.projection`` fed as the reference feeds it
  * ``fit_buffers(renderer, pose, proj, h, w)``   the render up to its antialiased buffers: ``FitBuffers``
  * ``fit_loss(buffers, rgb, mask, ...)``   clamp, composite, view cosine, the three masks and the MSE: 0-dim
  * ``fit_texture(renderer, views, ...)``   the loop; ``NeTFRenderer.fit_texture_from_mesh`` is this function

The reference states the loss as ``MSELoss(image[m], flipud(rgb)[m])`` on the output of ``render``: some twenty full-image
elementwise launches behind the kernels and a boolean gather that waits for the GPU.  Here a view is two launches forward
and one backward, every sum has a fixed order and nothing synchronises with the host.  The gradient reaches ``c_aa`` only:
alpha, position, normal and the targets carry none (fixed geometry), and one of them requiring a gradient raises.  A view
that selects no pixel gives loss 0 and a zero gradient (the reference: NaN).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _native
from ._launch import launch, require_gpu, scratch
from .mesh_losses import _image as _loss_image
from .mesh_render import antialias, antialias_weights, interpolate, projection, rasterize


class FitView(NamedTuple):
    c2w: np.ndarray        # [4,4]: the captured view's camera-to-world matrix
    K: np.ndarray          # [3,3]: its pinhole intrinsics
    rgb: torch.Tensor      # float32 [H,W,3] on the GPU
    mask: torch.Tensor     # float32 [H,W,1] or [H,W] on the GPU


class FitBuffers(NamedTuple):
    c_aa: torch.Tensor     # float32 [H,W,3]: antialiased colour, before the clamp; the one that carries a gradient
    a_aa: torch.Tensor     # float32 [H,W]: antialiased alpha, before its second clamp
    p_aa: torch.Tensor     # float32 [H,W,3]: antialiased position
    n_aa: torch.Tensor     # float32 [H,W,3]: antialiased, unnormalised normal
    center: torch.Tensor   # float32 [3]: the camera's centre, world space


def _normalized(x: np.ndarray) -> np.ndarray:
    """kiui.op.safe_normalize on the host"""
    return x / np.sqrt(np.maximum(np.sum(x * x), 1e-20))


def fit_pose(c2w) -> np.ndarray:
    """float32 [4,4]: the pose the reference renders a captured view with (mesh_renderer.py:176-213), operation for
    operation: the camera position permuted to ``(t_y, t_z, t_x)``, kiui's OpenGL ``look_at`` towards the origin (columns
    ``[right, up, forward]``, ``forward = normalize(campos)``), then four sign flips on axes 0, 2, 0, 2, each of which
    negates that component of the position and of columns 1 and 2 and rebuilds column 0 as ``normalize(cross(col2,
    col1))``.  The flips cancel in the position and in columns 1 and 2; what is left is the rotation
    ``[-right, up, forward]`` (determinant -1: a mirrored camera) at ``(t_y, t_z, t_x)``."""
    c2w = np.asarray(c2w, dtype=np.float64)
    if c2w.shape != (4, 4):
        raise ValueError("fit_pose: c2w must be [4,4]")
    t = c2w[:3, 3]
    position = np.array([t[1], t[2], t[0]])
    forward = _normalized(position)
    right = _normalized(np.cross(np.array([0.0, 1.0, 0.0]), forward))
    if not np.isfinite(position).all() or not np.any(right):
        raise ValueError("fit_pose: the permuted camera position must be finite and off the y axis")
    up = _normalized(np.cross(forward, right))
    rotation = np.stack([right, up, forward], axis=1)
    for axis in (0, 2, 0, 2):
        position[axis] = -position[axis]
        rotation[axis, 1] = -rotation[axis, 1]
        rotation[axis, 2] = -rotation[axis, 2]
        column = np.cross(rotation[:, 2], rotation[:, 1])
        rotation[:, 0] = column / np.linalg.norm(column)
    pose = np.eye(4)
    pose[:3, :3] = rotation
    pose[:3, 3] = position
    return pose.astype(np.float32)


def fit_projection(K, width, height) -> np.ndarray:
    """float32 [4,4]: ``mesh_render.projection`` of the intrinsics ``K`` [3,3] (mesh_renderer.py:216-221, which passes the
    image's ``shape[0]`` as ``width`` and ``shape[1]`` as ``height``)."""
    K = np.asarray(K)
    if K.shape != (3, 3):
        raise ValueError("fit_projection: K must be [3,3]")
    return projection(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], width=int(width), height=int(height))


def fit_buffers(renderer, pose, proj, h, w) -> FitBuffers:
    """What ``renderer.render(pose, proj, h, w)`` (a ``NeTFRenderer``) hands to its tail, from the same ops in the same
    order: the matrices, rasterize, one silhouette analysis, ``v`` and ``vn`` interpolated, the field on every pixel with the
    coverage ``alpha > 0`` as its mask, and the four antialias calls.  ``depth``, ``normal`` and every elementwise op of the
    tail are left out: ``fit_loss`` does the tail."""
    h, w = int(h), int(w)
    v, f, topo = renderer.v, renderer.f, renderer.topology
    mats = renderer._matrices(pose, proj)
    _, v_clip = renderer._clip(mats)
    rast = rasterize(v_clip, f, (h, w))
    wts = antialias_weights(rast, v_clip, f, topo)
    a_aa = antialias(torch.clamp(rast[..., -1:], 0, 1).contiguous(), rast, v_clip, f, weights=wts)
    xyzs = interpolate(v, rast, f)
    color = renderer._texture(xyzs.view(-1, 3), (a_aa > 0).view(-1)).view(h, w, 3)     # clamp(a, 0, 1) > 0 is a > 0
    c_aa = antialias(color, rast, v_clip, f, weights=wts)
    with torch.no_grad():
        p_aa = antialias(xyzs, rast, v_clip, f, weights=wts)
        n_aa = antialias(interpolate(renderer.vn, rast, f), rast, v_clip, f, weights=wts)
        center = mats[2][:3, 3].contiguous()
    return FitBuffers(c_aa, a_aa[..., 0], p_aa, n_aa, center)


class _FitLoss(torch.autograd.Function):
    """(loss 0-dim, image [H,W,3], cosinesview [H,W], m uint8 [H,W]) of one view; the gradient goes to ``c_aa``"""

    @staticmethod
    def forward(ctx, c_aa, a_aa, p_aa, n_aa, center, rgb, tmask, bg, flip_rows):
        dev = c_aa.device
        H, W = c_aa.shape[0], c_aa.shape[1]
        image = torch.empty_like(c_aa)
        cosinesview = torch.empty((H, W), dtype=torch.float32, device=dev)
        m = torch.empty((H, W), dtype=torch.uint8, device=dev)
        stats = torch.empty(_native.FIT_STATS_WORDS, dtype=torch.float32, device=dev)
        launch("gd_fit_loss_forward", dev, H, W, flip_rows, c_aa, a_aa, p_aa, n_aa, center, rgb, tmask, bg, image,
               cosinesview, m, stats, scratch(_native.lib().gd_fit_loss_scratch_bytes(H * W), dev))
        ctx.save_for_backward(c_aa, a_aa, rgb, bg, m, stats)
        ctx.flip_rows = flip_rows
        ctx.mark_non_differentiable(image, cosinesview, m)
        return stats[0], image, cosinesview, m

    @staticmethod
    def backward(ctx, dloss, *_):
        c_aa, a_aa, rgb, bg, m, stats = ctx.saved_tensors
        dc_aa = torch.empty_like(c_aa)
        launch("gd_fit_loss_backward", c_aa.device, c_aa.shape[0], c_aa.shape[1], ctx.flip_rows, c_aa, a_aa, rgb, bg, m,
               stats, dloss.reshape(1).to(torch.float32).contiguous(), dc_aa)
        return dc_aa, None, None, None, None, None, None, None, None


def _image(what: str, t, channels: int, like: Optional[torch.Tensor] = None, fixed: bool = True) -> torch.Tensor:
    """``mesh_losses``' image check (contiguous float32 on the GPU, [H,W,3] or [H,W] from [H,W,1], of ``like``'s resolution),
    then: ``fixed``, it may not require a gradient; and it starts on a 16-byte boundary (a copy if it does not)"""
    t = _loss_image("fit_loss", what, t, channels, like)
    if fixed and t.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"fit_loss: there is no gradient to {what}: detach it (the fit keeps the geometry and the "
                                  "targets fixed)")
    return t if t.data_ptr() % 16 == 0 else t.clone()


def background(bg_color, device) -> torch.Tensor:
    """float32 [3] on ``device`` of a number, three numbers or a tensor; a number costs one fill and no copy from the host"""
    if isinstance(bg_color, torch.Tensor):
        bg = require_gpu("fit_loss", "bg_color", bg_color, torch.float32).detach().reshape(-1)
        if bg.numel() not in (1, 3):
            raise ValueError("fit_loss: bg_color must be one number or three")
        return bg.expand(3).contiguous()
    if np.ndim(bg_color) == 0:
        return torch.full((3,), float(bg_color), dtype=torch.float32, device=device)
    host = torch.tensor([float(x) for x in bg_color], dtype=torch.float32)
    if host.numel() != 3:
        raise ValueError("fit_loss: bg_color must be one number or three")
    return host.pin_memory().to(device, non_blocking=True)


def fit_loss(buffers: FitBuffers, rgb: torch.Tensor, mask: torch.Tensor, bg_color=1.0, flip_rows: bool = True,
             outputs: bool = False):
    """The fit's loss of one view (include/gd_fit.h): ``image = a c + (1 - a) bg`` of the clamped buffers, the cosine of the
    view direction with the normal, ``m = (a > 0) & (mask > 0) & (cos <= 0)`` and the MSE between ``image`` and ``rgb`` over
    ``m``; ``flip_rows`` reads the targets upside down (the reference's ``torch.flipud``).  0-dim, and with ``outputs`` the
    tuple (loss, ``image`` [H,W,3], ``cosinesview`` [H,W], ``m`` uint8 [H,W]).  ``buffers``: ``fit_buffers(...)`` or any five
    tensors of those shapes."""
    if len(buffers) != 5:
        raise ValueError("fit_loss: buffers must be (c_aa, a_aa, p_aa, n_aa, center)")
    c_aa = _image("c_aa", buffers[0], 3, fixed=False)
    a_aa = _image("a_aa", buffers[1], 1, c_aa)
    p_aa = _image("p_aa", buffers[2], 3, c_aa)
    n_aa = _image("n_aa", buffers[3], 3, c_aa)
    center = require_gpu("fit_loss", "center", buffers[4], torch.float32)
    if center.numel() != 3:
        raise ValueError("fit_loss: center must be [3]")
    if center.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("fit_loss: there is no gradient to center: detach it")
    rgb = _image("rgb", rgb, 3, c_aa)
    mask = _image("mask", mask, 1, c_aa)
    bg = background(bg_color, c_aa.device)
    out = _FitLoss.apply(c_aa, a_aa.detach(), p_aa.detach(), n_aa.detach(), center.detach().reshape(3).contiguous(),
                         rgb.detach(), mask.detach(), bg, int(bool(flip_rows)))
    return out if outputs else out[0]


def fit_texture(renderer, views: Sequence[FitView], iters=600, resolution=1024, hashgrid_lr=0.01, mlp_lr=0.001, seed=0,
                save_path=None, optimizer=None) -> torch.Tensor:
    """``Renderer.fit_texture_from_mesh``: ``iters`` Adam steps of ``renderer.texture_fn`` (a ``TextureField``) on the MSE
    between the render at ``resolution`` and one captured view per step, drawn by a host generator seeded with ``seed``.
    Returns the loss history as ONE float32 device tensor [iters]; no iteration waits for the GPU.  ``optimizer``: a
    ``TextureFieldOptimizer`` to go on with (a new one with the two learning rates otherwise).  With ``save_path`` the
    run ends in ``renderer.export_mesh(save_path, reverse=True)``, as the reference's does."""
    from .texture_field import TextureField
    if len(views) == 0:
        raise ValueError("fit_texture_from_mesh: at least one view")
    if optimizer is None:
        if not isinstance(renderer.texture_fn, TextureField):
            raise TypeError("fit_texture_from_mesh: texture_fn must be a TextureField (or pass optimizer=)")
        optimizer = renderer.texture_fn.optimizer(hashgrid_lr, mlp_lr)
    iters, resolution = int(iters), int(resolution)
    cameras = []
    for view in views:
        require_gpu("fit_texture_from_mesh", "view.rgb", view.rgb, torch.float32)
        cameras.append((fit_pose(view.c2w), fit_projection(view.K, view.rgb.shape[0], view.rgb.shape[1])))
    dev = renderer.v.device
    history = torch.zeros(max(iters, 0), dtype=torch.float32, device=dev)
    bg = background(1.0, dev)
    rng = np.random.default_rng(seed)
    optimizer.zero_grad()
    for i in range(iters):
        k = int(rng.integers(len(views)))
        pose, proj = cameras[k]
        loss = fit_loss(fit_buffers(renderer, pose, proj, resolution, resolution), views[k].rgb, views[k].mask, bg)
        loss.backward()
        optimizer.step()
        optimizer.zero_grad()
        history[i].copy_(loss.detach())
    if save_path is not None:
        renderer.export_mesh(save_path, reverse=True)
    return history
