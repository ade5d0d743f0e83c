"""G-buffer losses of the mesh deformer's second stage (stage 3 of the reference: ``deformer/losses/normal.py``,
``losses/mask.py``) on the HIP kernels of ``csrc/raster_gbuffer_losses.hip`` (C-ABI and definitions:
include/gd_mesh_losses.h) -- no CPU path.

  * ``normal_map_loss_enhanced(views, gbuffers, epsilon=-0.1)``   <- ``normal_map_loss_enhanced``
  * ``normal_map_loss(views, gbuffers)``                          <- ``normal_map_loss`` with its default L1
  * ``hole_mask_loss(views, gbuffers, gbuffers_rf)``              <- ``hole_mask_loss`` with its default MSE
  * ``second_stage_losses(views, gbuffers, gbuffers_rf)``         all three from one forward and one backward per view
  * ``shading_loss(views, gbuffers, shader, shading_percentage)`` <- ``losses/shading.py`` over a ``neural_shader.NeuralShader``
    (include/gd_shader.h; ``csrc/raster_shader.hip``, ``csrc/raster_shader_mfma.hip``)

A view is a ``View`` of GPU tensors; a G-buffer is the dict ``GBufferRenderer.render`` returns, with ``mask`` [H,W,1],
``position`` and ``normal`` [H,W,3].  Each loss is the mean over the views of the per-view term.  Gradients reach
``gbuffer["normal"]`` (all three terms) and ``gbuffer["position"]`` (the hole-mask term only: the reference overwrites the
data of its cosine with the sign, so autograd differentiates the cosine); masks, targets and the ``_rf`` side receive none.
The shading loss sends gradients to ``position`` (through the encoding and the view direction) and ``normal``, and adds
those of the shader's parameters into the shader's flat gradient buffer.

The reference states each term as some thirty elementwise ops ending in a boolean-mask gather, which waits for the GPU;
here a view is two launches forward and one backward, every sum has a fixed order, and nothing synchronises with the host.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Sequence

import torch

from . import _native
from ._launch import launch, require_gpu, scratch

ENHANCED, PLAIN, HOLE = _native.MESH_LOSS_ENHANCED, _native.MESH_LOSS_PLAIN, _native.MESH_LOSS_HOLE
DEFAULT_EPSILON = -0.1


class View(NamedTuple):
    normal: torch.Tensor    # float32 [H,W,3] in [0,1]: the view's estimated normal map, camera space
    mask: torch.Tensor      # float32 [H,W,1] or [H,W]
    R: torch.Tensor         # float32 [3,3]: the camera's rotation
    center: torch.Tensor    # float32 [3]: the camera's centre, world space
    rgb: Optional[torch.Tensor] = None    # float32 [H,W,3]: the view's image, read by shading_loss only


class _GBufferLosses(torch.autograd.Function):
    """(enhanced, plain, hole) of one view as a float32 [3]; the terms outside ``terms`` are 0."""

    @staticmethod
    def forward(ctx, normal, position, mask, rf, target_normal, target_mask, camera, epsilon, terms):
        dev = normal.device
        H, W = normal.shape[0], normal.shape[1]
        stats = torch.empty(_native.MESH_LOSS_STATS_WORDS, dtype=torch.float32, device=dev)
        eps = C.c_float(epsilon)
        launch("gd_mesh_gbuffer_losses_forward", dev, H, W, terms, normal, position, mask, *rf, target_normal,
               target_mask, camera, eps, stats,
               scratch(_native.lib().gd_mesh_gbuffer_losses_scratch_bytes(H * W), dev))
        ctx.save_for_backward(normal, position, mask, *rf, target_normal, target_mask, camera, stats)
        ctx.epsilon, ctx.terms = eps, terms
        return stats[:3]

    @staticmethod
    def backward(ctx, dloss):
        *inputs, camera, stats = ctx.saved_tensors      # a buffer the enabled terms do not read is None
        normal, position = inputs[0], inputs[1]
        dnormal, dposition = torch.empty_like(normal), torch.empty_like(position)
        launch("gd_mesh_gbuffer_losses_backward", normal.device, normal.shape[0], normal.shape[1], ctx.terms, *inputs,
               camera, ctx.epsilon, stats, dloss.contiguous(), dnormal, dposition)
        return dnormal, (dposition if ctx.terms & HOLE else None), None, None, None, None, None, None, None


def _image(name: str, what: str, t, channels: int, like: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``t`` as a contiguous float32 GPU image: [H,W,3], or [H,W] from [H,W,1] / [H,W]; of ``like``'s H x W if given."""
    require_gpu(name, what, t, torch.float32)
    if channels == 1 and t.dim() == 3 and t.shape[-1] == 1:
        t = t[..., 0]
    if t.dim() != (3 if channels == 3 else 2) or (channels == 3 and t.shape[-1] != 3):
        raise ValueError(f"{name}: {what} must be [H,W,{channels}]")
    if like is not None and tuple(t.shape[:2]) != tuple(like.shape[:2]):
        raise ValueError(f"{name}: {what} must have the resolution of the G-buffer")
    return t.contiguous()


def _gbuffer(name: str, what: str, g, like: Optional[torch.Tensor] = None):
    normal = _image(name, f"{what}['normal']", g["normal"], 3, like)
    return normal, _image(name, f"{what}['position']", g["position"], 3, normal), \
        _image(name, f"{what}['mask']", g["mask"], 1, normal)


def camera_block(view: View) -> torch.Tensor:
    """float32 [12] on the GPU: ``R`` row-major, then ``center`` -- what the kernels read; the host never does."""
    R = require_gpu("mesh_losses", "view.R", view.R, torch.float32)
    center = require_gpu("mesh_losses", "view.center", view.center, torch.float32)
    if tuple(R.shape) != (3, 3) or center.numel() != 3:
        raise ValueError("mesh_losses: view.R must be [3,3] and view.center [3]")
    return torch.cat((R.reshape(9), center.reshape(3)))


def view_losses(view: View, gbuffer, gbuffer_rf=None, terms: int = ENHANCED | PLAIN | HOLE,
                epsilon: float = DEFAULT_EPSILON, camera: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [3] = (enhanced, plain, hole) of ONE view from one fused call; a term outside ``terms`` is 0.  ``camera``: the
    view's ``camera_block`` if the caller keeps one (it is built here otherwise)."""
    name = "mesh_losses"
    if not 0 < terms <= (ENHANCED | PLAIN | HOLE):
        raise ValueError("mesh_losses: terms must be a non-empty subset of ENHANCED | PLAIN | HOLE")
    normal, position, mask = _gbuffer(name, "gbuffer", gbuffer)
    rf = (None, None, None)
    if terms & HOLE:
        if gbuffer_rf is None:
            raise ValueError("mesh_losses: the hole-mask loss needs the reference mesh's G-buffer")
        rf = tuple(t.detach() for t in _gbuffer(name, "gbuffer_rf", gbuffer_rf, normal))
    target_normal = target_mask = None
    if terms & (ENHANCED | PLAIN):
        target_normal = _image(name, "view.normal", view.normal, 3, normal).detach()
        target_mask = _image(name, "view.mask", view.mask, 1, normal).detach()
    camera = camera_block(view) if camera is None else require_gpu(name, "camera", camera, torch.float32)
    if camera.numel() != 12 or not camera.is_contiguous():
        raise ValueError("mesh_losses: camera must be 12 contiguous floats")
    return _GBufferLosses.apply(normal, position, mask.detach(), rf, target_normal, target_mask, camera.detach(),
                                float(epsilon), int(terms))


def _mean_over_views(views: Sequence[View], gbuffers, gbuffers_rf, terms: int, epsilon: float, cameras=None) -> torch.Tensor:
    if len(views) == 0 or len(views) != len(gbuffers) or (gbuffers_rf is not None and len(gbuffers_rf) != len(views)):
        raise ValueError("mesh_losses: one G-buffer per view, and at least one view")
    total = None
    for k, (view, gbuffer) in enumerate(zip(views, gbuffers)):
        one = view_losses(view, gbuffer, None if gbuffers_rf is None else gbuffers_rf[k], terms, epsilon,
                          None if cameras is None else cameras[k])
        total = one if total is None else total + one
    return total / len(views)


def normal_map_loss_enhanced(views: Sequence[View], gbuffers, epsilon: float = DEFAULT_EPSILON) -> torch.Tensor:
    """Mean over the views of ``sum_in (1 - cos(t, n_cam)) w / Z`` (include/gd_mesh_losses.h, ENHANCED).  0-dim."""
    return _mean_over_views(views, gbuffers, None, ENHANCED, epsilon)[0]


def normal_map_loss(views: Sequence[View], gbuffers) -> torch.Tensor:
    """Mean over the views of the L1 distance between ``0.5 (n_cam + 1)`` and the normal map over the pixels both masks
    cover (PLAIN); a view without such a pixel adds 0 (the reference: NaN).  0-dim."""
    return _mean_over_views(views, gbuffers, None, PLAIN, DEFAULT_EPSILON)[1]


def hole_mask_loss(views: Sequence[View], gbuffers, gbuffers_rf) -> torch.Tensor:
    """Mean over the views of the MSE between the facing signs of the mesh and of the reference mesh over the pixels both
    cover (HOLE), with the reference's straight-through gradient to ``normal`` and ``position``.  0-dim."""
    return _mean_over_views(views, gbuffers, gbuffers_rf, HOLE, DEFAULT_EPSILON)[2]


def second_stage_losses(views: Sequence[View], gbuffers, gbuffers_rf, enhanced: bool = True,
                        epsilon: float = DEFAULT_EPSILON, cameras=None) -> Dict[str, torch.Tensor]:
    """``{"normal_enhanced", "normal_plain", "hole_mask", "normal"}`` from ONE forward (two launches) and ONE backward (one
    launch) per view; ``normal`` is the enhanced loss or the plain one, as the reference's ``enhanced_normal_map_loss``
    switch selects."""
    out = _mean_over_views(views, gbuffers, gbuffers_rf, ENHANCED | PLAIN | HOLE, epsilon, cameras)
    losses = {"normal_enhanced": out[0], "normal_plain": out[1], "hole_mask": out[2]}
    losses["normal"] = losses["normal_enhanced" if enhanced else "normal_plain"]
    return losses


# ---- the shading loss over the neural shader ------------------------------------------------------------------------------

class _Shading(torch.autograd.Function):
    """The shading loss of one view (0-dim).  ``params`` are the shader's parameters: they make the result require a
    gradient and receive None, their gradients are ADDED into the shader's flat gradient buffer by the kernels."""

    @staticmethod
    def forward(ctx, position, normal, mask, view_mask, rgb, camera, shader, p, seed, step, capacity, record, *params):
        from . import neural_shader as ns
        dev = position.device
        H, W = position.shape[0], position.shape[1]
        cap = C.c_int64(capacity)
        rows = ns.rows_of(capacity)
        index = torch.empty(capacity, dtype=torch.int32, device=dev)
        counters = torch.empty(4, dtype=torch.int32, device=dev)
        act = torch.empty(rows * ns.ACT_WIDTH, dtype=torch.bfloat16, device=dev)
        logits = torch.empty(rows, 3, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        work = ns.workspace(capacity, dev)
        launch("gd_shader_select", dev, H, W, normal, position, mask, view_mask, camera, C.c_float(p), C.c_uint32(seed),
               C.c_uint32(step), cap, index, counters, scratch(_native.lib().gd_shader_select_scratch_bytes(H * W), dev))
        launch("gd_shader_features", dev, H, W, position, normal, camera, cap, index, counters, act)
        shader.forward_layers(capacity, counters, act, logits)
        launch("gd_shader_l1_forward", dev, H, W, cap, index, counters, logits, rgb, loss, work)
        ctx.save_for_backward(position, camera, index, counters, act, logits, rgb)
        ctx.shader, ctx.capacity, ctx.work = shader, capacity, work
        record.update(index=index, counters=counters, logits=logits)
        return loss[0]

    @staticmethod
    def backward(ctx, dloss):
        from . import neural_shader as ns
        position, camera, index, counters, act, logits, rgb = ctx.saved_tensors
        shader, capacity = ctx.shader, ctx.capacity
        dev = position.device
        H, W = position.shape[0], position.shape[1]
        cap = C.c_int64(capacity)
        rows = ns.rows_of(capacity)
        dz = torch.empty(rows * ns.DZ_WIDTH, dtype=torch.bfloat16, device=dev)
        dfeat = torch.empty(rows, 32, dtype=torch.float32, device=dev)
        dextra = torch.empty(rows, 32, dtype=torch.float32, device=dev)
        launch("gd_shader_l1_backward", dev, H, W, cap, index, counters, logits, rgb,
               dloss.reshape(1).to(torch.float32).contiguous(), dz, None)
        for l in range(ns.LAYERS - 1, -1, -1):
            launch("gd_shader_backward_weight_layer", dev, l, cap, counters, act, dz, shader.flat_grad, ctx.work)
            launch("gd_shader_backward_input_layer", dev, l, cap, counters, shader.packed_t, act, dz, dfeat, dextra)
        dposition, dnormal = torch.empty_like(position), torch.empty_like(position)
        launch("gd_shader_features_backward", dev, H, W, position, camera, cap, index, counters, dfeat, dextra, dposition,
               dnormal)
        return (dposition, dnormal) + (None,) * (10 + len(ctx.shader.parameters()))


def shading_loss(views: Sequence[View], gbuffers, shader, shading_percentage: float = 1.0, seed: int = 0, step: int = 0,
                 capacity: Optional[int] = None) -> torch.Tensor:
    """Mean over the views of the L1 distance between ``shader(position, normal, view_dir)`` and ``view.rgb`` over a sample
    of the pixels that both masks cover and that face the camera (include/gd_shader.h).  0-dim.  A valid pixel is kept when
    ``hash32(seed, step, pixel) < shading_percentage 2^32``: the number kept is binomial around ``shading_percentage`` of the
    valid pixels, where the reference keeps exactly ``int(n p)`` drawn by the host's ``randperm`` -- a stated deviation, paid
    for by not waiting for the GPU.  At most ``capacity`` pixels (``H W`` by default) are shaded, the first in pixel order;
    the rest is counted.  Gradients reach ``gbuffer["position"]`` and ``gbuffer["normal"]``; those of the shader's parameters
    are ADDED into ``shader.flat_grad``.  A view that keeps nothing adds 0 (the reference: NaN).

    After a call ``shading_loss.count`` and ``shading_loss.dropped`` hold int32 [views] device tensors, and
    ``shading_loss.last`` per view the index list, the counters and the logits of the shaded points."""
    from .neural_shader import NeuralShader, check_capacity
    name = "shading_loss"
    if not isinstance(shader, NeuralShader):
        raise TypeError(f"{name}: shader must be a neural_shader.NeuralShader")
    if len(views) == 0 or len(views) != len(gbuffers):
        raise ValueError(f"{name}: one G-buffer per view, and at least one view")
    p = float(shading_percentage)
    if not p >= 0.0:
        raise ValueError(f"{name}: shading_percentage must not be negative")
    if not (0 <= int(seed) < 1 << 32 and 0 <= int(step) < 1 << 32):
        raise ValueError(f"{name}: seed and step must fit 32 bits")
    params = shader.parameters()
    total, records = None, []
    for view, gbuffer in zip(views, gbuffers):
        if view.rgb is None:
            raise ValueError(f"{name}: the view has no rgb image (View(normal, mask, R, center, rgb))")
        if not isinstance(view.rgb, torch.Tensor) or view.rgb.dim() != 3 or view.rgb.shape[-1] != 3:
            raise ValueError(f"{name}: view.rgb must be [H,W,3]")
        normal, position, mask = _gbuffer(name, "gbuffer", gbuffer)
        rgb = _image(name, "view.rgb", view.rgb, 3, normal).detach()
        view_mask = _image(name, "view.mask", view.mask, 1, normal).detach()
        H, W = normal.shape[0], normal.shape[1]
        cap = check_capacity(name, H * W if capacity is None else capacity)
        record = {}
        one = _Shading.apply(position, normal, mask.detach(), view_mask, rgb, camera_block(view).detach(), shader, p,
                             int(seed), int(step), cap, record, *params)
        records.append(record)
        total = one if total is None else total + one
    shading_loss.last = records
    counters = torch.stack([r["counters"] for r in records])
    shading_loss.count, shading_loss.dropped = counters[:, 0], counters[:, 1]
    return total / len(views)
