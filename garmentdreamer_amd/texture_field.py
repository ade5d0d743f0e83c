"""The NeTF stage's texture field: ``color = sigmoid(mlp(encoder(xyz)))`` of ``Renderer.render``
(Garment_Deformer_NeTF/netf/render/mesh_renderer.py:368-375), with the multiresolution hash grid of
netf/render/texture_encoder.py:8-37 (tiny-cuda-nn's "Grid"/"Hash", linear interpolation) on the HIP kernels of
``csrc/raster_texture.hip`` (C-ABI and definitions: include/gd_texture.h) -- no CPU path.

  * ``grid_layout(...)``      the level table (numpy, float64), handed to the kernels by value
  * ``HashGridEncoder``       the reference's module: ``forward(x, bound=1)`` -> [N, 32]
  * ``TextureField``          the fused field, ``forward(x, mask=None)`` -> [N, 3]; ``.encoder`` / ``.mlp`` are the unfused
                              pair over the same parameters; ``optimizer()`` steps grid and MLP with one launch
  * ``NeTFRenderer``          ``MeshRenderer`` that evaluates a field on every pixel with the coverage as ``mask``: no
                              ``mask.any()``, no boolean indexing, nothing that waits for the GPU
                              ``export_mesh`` bakes the field into a UV atlas and writes the textured OBJ
                              (``texture_bake.py``); ``fit_texture_from_mesh`` fits the field to captured views
                              (``texture_fit.py``)

Gradients follow ``.grad`` semantics at the C level (every kernel ADDS into the buffer it is given).  A parameter that
``TextureFieldOptimizer`` has re-seated carries ``_gd_grad_sink`` (a view of the optimizer's flat gradient buffer, as
``flat_adam.FlatAdam`` gives the LoRA adapters): the backward adds straight into it and returns nothing to autograd.
Without a sink the backward allocates a zeroed gradient and returns it.

The gradient to ``x`` is opt-in (``position_gradient=True`` on ``encode``, ``field``, ``HashGridEncoder``, ``TextureField``;
kernels and definition: include/gd_texture_position.h): the derivative of the trilinear interpolation inside the cell the
forward chose, written (not added) by the same pass that forms the other gradients, no atomics, bit-reproducible; no double
backward.  It is what ``netf_geometry.DeformableNeTFRenderer`` (``fix_geo: false``) moves the vertices with.  Without the
flag, the live configuration's ``fix_geo: true``, nothing changes: ``x.requires_grad`` raises.  With the flag and an ``x`` that
needs no gradient the launches are the ones without it.

Determinism.  Every forward and the MLP gradients are bit-reproducible.  The gradient to the grid is by default accumulated
with float atomics (as tiny-cuda-nn does): its last bits differ between runs.  ``deterministic=True`` (``encode``, ``field``,
``HashGridEncoder``, ``TextureField``) routes the backward through the sorted path of include/gd_texture_sorted.h instead: a
stable sort of the contributions by grid entry and one sequential sum per entry in ascending (point, corner) order, no float
atomics; the grid gradient is then a pure function of the inputs, and two runs from the same seed stay bit-equal.  The
forwards are the same either way; the path needs ``N <= 2^24`` points per call and scratch that grows with N.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _native
from ._launch import launch, require_gpu, scratch
from .flat_adam import padded, reseat
from .mesh_render import MeshRenderer

FEATURES = 2
FIELD_WIDTH = 32
_X_GRAD = ("gradients with respect to the sample positions are not implemented: detach x, or keep the geometry fixed "
           "(fix_geo: true)")      # without position_gradient=True, that is (include/gd_texture_position.h)


class GridLayout(NamedTuple):
    num_levels: int
    scale: np.ndarray      # float32 [L]: s_l
    res: np.ndarray        # int64 [L]
    size: np.ndarray       # int64 [L], entries
    offset: np.ndarray     # int64 [L + 1], entries
    dense: np.ndarray      # bool [L]

    @property
    def num_entries(self) -> int:
        return int(self.offset[-1])

    @property
    def num_params(self) -> int:
        return self.num_entries * FEATURES

    @property
    def output_dim(self) -> int:
        return self.num_levels * FEATURES

    def struct(self) -> "_native.TextureLayout":
        s = _native.TextureLayout()
        s.num_levels = self.num_levels
        for l in range(self.num_levels):
            s.scale[l], s.res[l], s.size[l], s.offset[l] = float(self.scale[l]), int(self.res[l]), int(self.size[l]), \
                int(self.offset[l])
        s.offset[self.num_levels] = int(self.offset[-1])
        return s


def grid_layout(num_levels: int = 16, base_resolution: int = 16, per_level_scale: Optional[float] = None,
                log2_hashmap_size: int = 19, desired_resolution: int = 1024) -> GridLayout:
    """The level table of include/gd_texture.h.  ``per_level_scale`` defaults to the reference's
    ``exp2(log2(desired_resolution / num_levels) / (num_levels - 1))``."""
    if not 1 <= num_levels <= _native.TEXTURE_MAX_LEVELS:
        raise ValueError(f"grid_layout: num_levels must be in 1..{_native.TEXTURE_MAX_LEVELS}")
    if not 1 <= log2_hashmap_size <= 24:
        raise ValueError("grid_layout: log2_hashmap_size must be in 1..24")
    if base_resolution < 1:
        raise ValueError("grid_layout: base_resolution must be >= 1")
    if per_level_scale is None:
        per_level_scale = np.exp2(np.log2(desired_resolution / num_levels) / max(num_levels - 1, 1))
    if not per_level_scale >= 1.0:
        raise ValueError("grid_layout: per_level_scale must be >= 1")
    levels = np.arange(num_levels, dtype=np.float64)
    scale = (np.power(2.0, levels * np.log2(np.float64(per_level_scale))) * base_resolution - 1.0).astype(np.float32)
    res = np.ceil(scale.astype(np.float64)).astype(np.int64) + 1
    if res.max() > 1 << 21:
        raise ValueError("grid_layout: a level's resolution exceeds 2^21")
    size = np.minimum((res ** 3 + 7) // 8 * 8, 1 << log2_hashmap_size)
    offset = np.concatenate(([0], np.cumsum(size))).astype(np.int64)
    return GridLayout(num_levels, scale, res, size, offset, res ** 3 <= size)


def _points(name: str, x, mask, position_gradient: bool = False):
    """(x [N,3] contiguous, mask uint8 [N] or None); x is detached unless it requires a gradient and ``position_gradient``
    asks for one: then autograd sees it, and the backward returns ``dx`` to it"""
    require_gpu(name, "x", x, torch.float32)
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{name}: x must be [N,3]")
    wants_dx = x.requires_grad and torch.is_grad_enabled()
    if wants_dx and not position_gradient:
        raise NotImplementedError(f"{name}: " + _X_GRAD)
    if mask is not None:
        require_gpu(name, "mask", mask)
        if mask.numel() != x.shape[0]:
            raise ValueError(f"{name}: mask must have one element per point")
        mask = mask.reshape(-1)
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)          # same bytes: True is 1
        elif mask.dtype != torch.uint8:
            raise TypeError(f"{name}: mask must be bool or uint8")
        mask = mask.contiguous()
    return (x if wants_dx else x.detach()).contiguous(), mask


def _sinks(params):
    """``Parameter._gd_grad_sink`` of each (read in the forward: autograd hands the backward other tensor objects)"""
    return [getattr(p, "_gd_grad_sink", None) for p in params]


def _grad_targets(params, sinks):
    """per parameter: (buffer the kernel adds into, what autograd gets back)"""
    out = []
    for p, sink in zip(params, sinks):
        if sink is not None and sink.shape == p.shape and sink.is_contiguous():
            out.append((sink, None))
        else:
            g = torch.zeros_like(p, memory_format=torch.contiguous_format)
            out.append((g, g))
    return out


def _sort_scratch(n: int, struct, dev) -> torch.Tensor:
    """the sorted path's scratch; more than 2^24 points are refused here, before anything of that size is allocated"""
    if n > _native.TEXTURE_SORTED_MAX_POINTS:
        raise ValueError(f"deterministic=True takes at most 2^24 points per call ({n} given): use the atomic path or split "
                         "the batch")
    return scratch(_native.lib().gd_texture_sorted_scratch_bytes(n, struct), dev)


class _Encode(torch.autograd.Function):
    """``x`` reaches autograd only where ``_points`` let it (``position_gradient``): then the backward returns ``dx``"""

    @staticmethod
    def forward(ctx, x, mask, grid, layout, struct, deterministic):
        enc = torch.empty((x.shape[0], layout.output_dim), dtype=torch.float32, device=x.device)
        launch("gd_texture_encode_forward", x.device, x.shape[0], x, mask, grid, struct, enc)
        ctx.save_for_backward(x, mask, grid)
        ctx.struct, ctx.sinks, ctx.deterministic = struct, _sinks([grid]), deterministic
        return enc

    @staticmethod
    @once_differentiable
    def backward(ctx, denc):
        x, mask, grid = ctx.saved_tensors
        (buf, ret), = _grad_targets([grid], ctx.sinks)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            launch("gd_texture_encode_backward_pos", x.device, x.shape[0], x, mask, grid, ctx.struct, denc.contiguous(), dx)
        if ctx.deterministic:
            launch("gd_texture_encode_backward_sorted", x.device, x.shape[0], x, mask, denc.contiguous(), ctx.struct, buf,
                   _sort_scratch(x.shape[0], ctx.struct, x.device))
        else:
            launch("gd_texture_encode_backward", x.device, x.shape[0], x, mask, denc.contiguous(), ctx.struct, buf)
        return dx, None, ret, None, None, None


class _Field(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, grid, w1, b1, w2, b2, struct, deterministic):
        color = torch.empty((x.shape[0], 3), dtype=torch.float32, device=x.device)
        launch("gd_texture_field_forward", x.device, x.shape[0], x, mask, grid, struct, w1, b1, w2, b2, color)
        ctx.save_for_backward(x, mask, grid, w1, b1, w2, b2, color)
        ctx.struct, ctx.sinks, ctx.deterministic = struct, _sinks([grid, w1, b1, w2, b2]), deterministic
        return color

    @staticmethod
    @once_differentiable
    def backward(ctx, dcolor):
        x, mask, grid, w1, b1, w2, b2, color = ctx.saved_tensors
        dev = x.device
        n = x.shape[0]
        dcolor = dcolor.contiguous()
        targets = _grad_targets([grid, w1, b1, w2, b2], ctx.sinks)
        slab = scratch(_native.lib().gd_texture_field_backward_scratch_bytes(n), dev)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None        # the same pass writes it (..._pos entries)
        pos, extra = ("_pos", [dx]) if dx is not None else ("", [])
        if ctx.deterministic:
            denc = torch.empty((n, FIELD_WIDTH), dtype=torch.float32, device=dev)
            launch("gd_texture_field_backward_sorted" + pos, dev, n, x, mask, grid, ctx.struct, w1, b1, w2, b2, color,
                   dcolor, *[t[0] for t in targets], denc, *extra, slab, _sort_scratch(n, ctx.struct, dev))
        else:
            launch("gd_texture_field_backward" + pos, dev, n, x, mask, grid, ctx.struct, w1, b1, w2, b2, color, dcolor,
                   *[t[0] for t in targets], *extra, slab)
        return (dx, None) + tuple(t[1] for t in targets) + (None, None)


def _param(name: str, what: str, p: torch.Tensor, shape) -> torch.Tensor:
    require_gpu(name, what, p, torch.float32)
    if tuple(p.shape) != tuple(shape) or not p.is_contiguous():
        raise ValueError(f"{name}: {what} must be a contiguous {tuple(shape)} tensor")
    return p


def encode(x: torch.Tensor, grid: torch.Tensor, layout: GridLayout, mask: Optional[torch.Tensor] = None,
           deterministic: bool = False, position_gradient: bool = False) -> torch.Tensor:
    """``enc`` float32 [N, L F] of the points ``x`` [N,3] (in [-1, 1]^3; anything finite is defined) in the flat table
    ``grid``; rows with ``mask == 0`` or a non-finite coordinate are 0 and pass no gradient.  ``deterministic``: the
    gradient to ``grid`` by sort and sum instead of atomics (see the module's docstring).  ``position_gradient``: an ``x``
    that requires a gradient gets one (include/gd_texture_position.h) instead of raising."""
    _param("encode", "grid", grid, (layout.num_params,))
    x, mask = _points("encode", x, mask, bool(position_gradient))
    return _Encode.apply(x, mask, grid, layout, layout.struct(), bool(deterministic))


def field(x: torch.Tensor, grid: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
          layout: GridLayout, mask: Optional[torch.Tensor] = None, deterministic: bool = False,
          position_gradient: bool = False) -> torch.Tensor:
    """``color`` float32 [N,3] = sigmoid(W2 relu(W1 enc + b1) + b2), one launch; needs ``L F = 32``.  ``deterministic``:
    the gradient to ``grid`` by sort and sum instead of atomics (see the module's docstring).  ``position_gradient``: an
    ``x`` that requires a gradient gets one, from the same backward pass, instead of raising."""
    if layout.output_dim != FIELD_WIDTH:
        raise ValueError(f"field: the fused path needs num_levels * level_dim = {FIELD_WIDTH}")
    _param("field", "grid", grid, (layout.num_params,))
    _param("field", "w1", w1, (FIELD_WIDTH, FIELD_WIDTH))
    _param("field", "b1", b1, (FIELD_WIDTH,))
    _param("field", "w2", w2, (3, FIELD_WIDTH))
    _param("field", "b2", b2, (3,))
    x, mask = _points("field", x, mask, bool(position_gradient))
    return _Field.apply(x, mask, grid, w1, b1, w2, b2, layout.struct(), bool(deterministic))


class HashGridEncoder(nn.Module):
    """The reference's ``HashGridEncoder`` (texture_encoder.py:8-37): same signature, same ``per_level_scale``; ``params`` is
    the flat table in tiny-cuda-nn's order (level, entry, feature), uniform in [-1e-4, 1e-4].  ``deterministic`` (kept as
    ``.deterministic``): the gradient to ``params`` by sort and sum instead of atomics.  ``position_gradient`` (kept as
    ``.position_gradient``): ``x`` may require a gradient and gets one."""

    def __init__(self, input_dim=3, num_levels=16, level_dim=2, log2_hashmap_size=19, base_resolution=16,
                 desired_resolution=1024, interpolation="linear", generator: Optional[torch.Generator] = None,
                 deterministic: bool = False, position_gradient: bool = False):
        super().__init__()
        if input_dim != 3 or level_dim != FEATURES:
            raise NotImplementedError("HashGridEncoder: only input_dim=3 and level_dim=2 are built")
        if interpolation != "linear":
            raise NotImplementedError("HashGridEncoder: only linear interpolation is built (the reference never asks "
                                      "for smoothstep)")
        self._set_layout(grid_layout(num_levels, base_resolution, None, log2_hashmap_size, desired_resolution), generator,
                         deterministic, position_gradient)

    def _set_layout(self, layout: GridLayout, generator, deterministic=False, position_gradient=False):
        self.layout = layout
        self.deterministic = bool(deterministic)
        self.position_gradient = bool(position_gradient)
        self.input_dim = 3
        self.output_dim = layout.output_dim
        self.params = nn.Parameter((torch.rand(layout.num_params, generator=generator) * 2 - 1) * 1e-4)

    @classmethod
    def from_layout(cls, layout: GridLayout, generator: Optional[torch.Generator] = None,
                    deterministic: bool = False, position_gradient: bool = False) -> "HashGridEncoder":
        """An encoder over any ``grid_layout(...)`` (the constructor's arguments cannot state ``per_level_scale``)."""
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self._set_layout(layout, generator, deterministic, position_gradient)
        return self

    def forward(self, x, bound=1, mask=None):
        if bound != 1:
            raise ValueError("HashGridEncoder: only bound=1 is built")
        return encode(x, self.params, self.layout, mask, self.deterministic, self.position_gradient)


WEIGHT_GRAD_BLOCK = 128


def _blocked_outer(dy: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """``dy^T x`` [out,in] over the rows of ``dy`` [n,out] and ``x`` [n,in]: one small product per block of 128 rows, then
    the sum of the blocks.  ``nn.Linear``'s backward issues one GEMM ``dy.t().mm(x)``, a single running fp32 sum per entry
    over all n rows; the stage sums over ~10^5 pixels, where that sum is 4.0e-6 of the largest entry from float64 on
    MI355X and the blocked one 1.6e-7."""
    n = x.shape[0]
    if n == 0:
        return x.new_zeros(dy.shape[1], x.shape[1])
    blocks = (n + WEIGHT_GRAD_BLOCK - 1) // WEIGHT_GRAD_BLOCK
    pad = blocks * WEIGHT_GRAD_BLOCK - n
    if pad:
        dy, x = F.pad(dy, (0, 0, 0, pad)), F.pad(x, (0, 0, 0, pad))
    part = torch.bmm(dy.reshape(blocks, WEIGHT_GRAD_BLOCK, -1).transpose(1, 2), x.reshape(blocks, WEIGHT_GRAD_BLOCK, -1))
    return part.sum(dim=0)


class _BlockedLinear(torch.autograd.Function):
    """``F.linear`` on [..., in] whose weight gradient is ``_blocked_outer`` over all leading dimensions"""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dy @ weight if ctx.needs_input_grad[0] else None
        dy2 = dy.reshape(-1, dy.shape[-1])
        return dx, _blocked_outer(dy2, x.reshape(-1, x.shape[-1])), dy2.sum(dim=0)


class AlbedoMLP(nn.Module):
    """The reference's ``MLP(32, 3, 32, 2)`` (texture_encoder.py:93-112): two ``nn.Linear`` with a ReLU between; same
    parameters, same forward, the weight gradients summed in blocks (``_blocked_outer``).  Input [..., 32].  The gradients
    reach ``.grad`` through autograd; where ``TextureFieldOptimizer`` has made ``.grad`` a view of its flat buffer, autograd
    accumulates into that view in place (what ``FlatAdam`` relies on for its non-LoRA producers)."""

    def __init__(self, dim_in=FIELD_WIDTH, dim_out=3, dim_hidden=FIELD_WIDTH):
        super().__init__()
        self.net = nn.ModuleList([nn.Linear(dim_in, dim_hidden), nn.Linear(dim_hidden, dim_out)])

    def forward(self, x):
        l1, l2 = self.net
        return _BlockedLinear.apply(F.relu(_BlockedLinear.apply(x, l1.weight, l1.bias)), l2.weight, l2.bias)


class TextureField(nn.Module):
    """``sigmoid(mlp(encoder(x)))`` in one launch forward, and one launch plus the fixed-order sum backward.
    ``encoder``: a ``HashGridEncoder`` with ``output_dim == 32`` (default: the reference's).  ``generator`` seeds the grid;
    the MLP is ``nn.Linear``-initialised from torch's global generator.  ``deterministic``: if not ``None`` it is set on
    the encoder; ``forward``, ``unfused`` and ``.encoder(...)`` all follow ``encoder.deterministic``.
    ``position_gradient``: the same pattern, ``encoder.position_gradient``."""

    def __init__(self, encoder: Optional[HashGridEncoder] = None, generator: Optional[torch.Generator] = None,
                 deterministic: Optional[bool] = None, position_gradient: Optional[bool] = None):
        super().__init__()
        self.encoder = encoder if encoder is not None else HashGridEncoder(generator=generator)
        if deterministic is not None:
            self.encoder.deterministic = bool(deterministic)
        if position_gradient is not None:
            self.encoder.position_gradient = bool(position_gradient)
        if self.encoder.output_dim != FIELD_WIDTH:
            raise ValueError(f"TextureField: the fused path needs an encoder with output_dim = {FIELD_WIDTH}")
        self.mlp = AlbedoMLP()

    def forward(self, x, mask=None):
        l1, l2 = self.mlp.net
        return field(x, self.encoder.params, l1.weight, l1.bias, l2.weight, l2.bias, self.encoder.layout, mask,
                     self.encoder.deterministic, self.encoder.position_gradient)

    def unfused(self, x, mask=None):
        """The same function through ``.encoder`` and ``.mlp`` (the [N,32] encoding goes through memory)."""
        color = torch.sigmoid(self.mlp(self.encoder(x, mask=mask)))
        if mask is None:
            return color * torch.isfinite(x).all(dim=1, keepdim=True)
        return color * (torch.isfinite(x).all(dim=1) & (mask.reshape(-1) != 0))[:, None]

    def get_params(self, hashgrid_lr=0.01, mlp_lr=0.001):
        """The reference's two groups (mesh_renderer.py:248-253)."""
        return [{"params": list(self.encoder.parameters()), "lr": hashgrid_lr},
                {"params": list(self.mlp.parameters()), "lr": mlp_lr}]

    def optimizer(self, hashgrid_lr=0.01, mlp_lr=0.001, betas=(0.9, 0.999), eps=1e-8) -> "TextureFieldOptimizer":
        return TextureFieldOptimizer(self, hashgrid_lr, mlp_lr, betas, eps)


class TextureFieldOptimizer:
    """``torch.optim.Adam(field.get_params(...))`` as ONE ``gd_scene_adam_step`` launch over one flat buffer holding the
    grid and then the MLP, the two ranges with their own learning rate; ``zero_grad`` is ONE memset.  The parameters are
    re-seated as views of the flat buffer NOW and their ``.grad`` are, for good, views of the flat gradient buffer, into
    which the field's backward adds directly.  As with ``FlatAdam``: a parameter always has a gradient here (zeros if
    nothing wrote one), so its moments decay on every step."""

    def __init__(self, field_module: TextureField, hashgrid_lr=0.01, mlp_lr=0.001, betas=(0.9, 0.999), eps=1e-8):
        grid = [field_module.encoder.params]
        mlp = list(field_module.mlp.parameters())
        for p in grid + mlp:
            require_gpu("TextureFieldOptimizer", "every parameter", p, torch.float32)
        self._flat, self._grad, self._exp_avg, self._exp_avg_sq, _ = reseat(grid + mlp)
        self._ends = (C.c_int64 * 2)(padded(grid[0].numel()), self._flat.numel())
        self.param_groups = [{"params": grid, "lr": float(hashgrid_lr)}, {"params": mlp, "lr": float(mlp_lr)}]
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.step_count = 0

    def zero_grad(self, set_to_none: bool = False):
        self._grad.zero_()

    @torch.no_grad()
    def step(self):
        self.step_count += 1
        lrs = (C.c_double * 2)(float(self.param_groups[0]["lr"]), float(self.param_groups[1]["lr"]))
        launch("gd_scene_adam_step", self._flat.device, self._flat, self._grad, self._exp_avg, self._exp_avg_sq,
               self._flat.numel(), 2, self._ends, lrs, self.betas[0], self.betas[1], self.eps, self.step_count)


class NeTFRenderer(MeshRenderer):
    """``MeshRenderer`` for a field that takes the coverage as an argument: ``texture_fn(xyzs [H W,3], mask uint8 [H W])``
    -> [H W,3] with zeros where ``mask == 0`` (a ``TextureField``).  Same outputs as ``MeshRenderer.render``, bit for bit:
    the pose is inverted by the same device routine as ``torch.inverse`` but through ``torch.linalg.inv_ex``, which leaves
    the status on the device where ``torch.inverse`` reads it back (a host inverse differs from the device's in the last
    bit, and with it every barycentric), and the matrices go up in one asynchronous copy from pinned memory.  torch issues
    no synchronisation in a render, its backward and an optimizer step (``torch.cuda.set_sync_debug_mode("error")``); that
    mode sees torch's own synchronisation points, not a wait inside the solver library behind ``inv_ex``, which is not
    excluded by it.  A singular or non-finite pose raises, as in ``MeshRenderer``; it is detected on the host."""

    @classmethod
    def from_mesh(cls, vertices, indices, texture_fn, clean=True, min_faces=32, min_diameter_pct=10.0, **clean_args):
        """The renderer of a mesh as it was loaded (``Renderer.__init__``, mesh_renderer.py:114-121): with ``clean`` the
        mesh goes through ``mesh_clean.clean_mesh`` first, with the reference's ``min_f=32`` and ``min_d=10`` and
        ``clean_args`` for the rest; ``vn`` are ``mesh_geometry.normals`` of what is left.  ``vertices`` float32 [V,3] and
        ``indices`` [F,3] on the GPU; ``ValueError`` if cleaning leaves no face."""
        from . import mesh_clean, mesh_geometry
        v, f = vertices, indices
        if clean:
            cleaned = mesh_clean.clean_mesh(v, f, min_faces=min_faces, min_diameter_pct=min_diameter_pct, **clean_args)
            v, f = cleaned.vertices, cleaned.indices
            if f.shape[0] == 0:
                raise ValueError("NeTFRenderer.from_mesh: cleaning left no face of the mesh")
        v = require_gpu("NeTFRenderer.from_mesh", "vertices", v, torch.float32, 3).detach().contiguous()
        geo = mesh_geometry.build_geometry(f, v.shape[0], v.device)
        return cls(v, f, mesh_geometry.normals(v, geo)[1].detach(), texture_fn)

    def _matrices(self, pose, proj):
        """device float32 [3,4,4]: inverse pose, projection, pose"""
        pose = np.asarray(pose).astype(np.float32)
        try:
            ok = bool(np.isfinite(np.linalg.inv(pose)).all())
        except np.linalg.LinAlgError:
            ok = False
        if not ok:
            raise torch.linalg.LinAlgError("NeTFRenderer: the pose is singular or not finite")
        mats = np.stack([pose, np.asarray(proj)]).astype(np.float32)
        mats = torch.from_numpy(mats).pin_memory().to(self.v.device, non_blocking=True)
        return torch.stack([torch.linalg.inv_ex(mats[0]).inverse, mats[1], mats[0]])

    def _texture(self, xyzs, mask):
        return self.texture_fn(xyzs, mask).float()

    def fit_texture_from_mesh(self, views, iters=600, resolution=1024, hashgrid_lr=0.01, mlp_lr=0.001, seed=0,
                              save_path=None, optimizer=None):
        """``Renderer.fit_texture_from_mesh`` (mesh_renderer.py:158-240): ``iters`` Adam steps on the masked MSE between the
        render and one of ``views`` (``texture_fit.FitView``) per step; returns the loss history as one device tensor
        [iters].  See ``texture_fit.fit_texture``."""
        from . import texture_fit
        return texture_fit.fit_texture(self, views, iters, resolution, hashgrid_lr, mlp_lr, seed, save_path, optimizer)

    def export_mesh(self, save_path, texture_resolution=2048, padding=16, reverse=False, vt=None, ft=None, atlas="grid"):
        """``Renderer.export_mesh`` (mesh_renderer.py:260-313) plus optional UVs: bakes ``texture_fn`` into the atlas ``vt`` /
        ``ft`` (if not given: ``texture_bake.grid_atlas`` of the mesh for ``atlas="grid"``, one chart per triangle and
        seam-heavy; ``texture_atlas.chart_atlas`` for ``atlas="chart"``) and writes ``save_path`` with its ``.mtl`` and
        ``_albedo.png``; returns the three paths.  Waits for the GPU (once per run)."""
        from . import texture_bake
        return texture_bake.export_textured_mesh(save_path, self.texture_fn, self.v, self.f, texture_resolution, padding,
                                                 reverse, vt, ft, atlas)
