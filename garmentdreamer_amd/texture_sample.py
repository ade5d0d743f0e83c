"""Texture sampling for the mesh path: what a textured render needs beyond ``mesh_render`` -- nvdiffrast's fourth
operation ``dr.texture`` and the two things it rests on, the screen-space derivatives of ``dr.rasterize`` (``rast_db``) and
of ``dr.interpolate(..., rast_db=, diff_attrs='all')`` -- on the HIP kernels of ``csrc/raster_sample.hip`` (C-ABI and
definitions: include/gd_sample.h); no CPU path.

  * ``rast_derivatives(rast, pos, tri)``                     ``rast_db`` [H,W,4] = (du/dX, du/dY, dv/dX, dv/dY)
  * ``interpolate_derivatives(attr, rast, rast_db, tri)``    [H,W,2C]: per channel (d/dX, d/dY)
  * ``build_mipmaps(tex, max_mip_level)``                    the mip pyramid, built once and shared between calls
  * ``texture(tex, uv, uv_da, ...)``                         nearest / linear / linear-mipmap-nearest / linear-mipmap-linear,
                                                             wrap / clamp; gradient to ``tex`` (bit-reproducible, no atomics)
  * ``render_mesh(...)``                                     the reference's ``render_mesh`` for ``ssaa = 1``
                                                             (Garment_Deformer_NeTF/netf/render/mesh_renderer.py:18-103)
  * ``load_textured_obj(path)``                              reads back what ``texture_bake.write_textured_obj`` wrote

nvdiffrast is not available to this project: the agreement of these definitions with it is unverified (the level rule is
its published one).  Not built: a gradient to ``uv`` / ``uv_da``, the ``cube`` and ``zero`` boundary modes, a mip bias,
``ssaa``.  Texture row 0 is ``v = 0`` (the package's atlas convention, ``texture_bake``)."""
from __future__ import annotations

import ctypes
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _mesh_ops as ops
from . import _native
from . import mesh_render as mr
from ._launch import launch, require_gpu
from .export import load_image_rgb
from .template import load_obj_uv

_UV_GRAD = ("gradients with respect to uv and uv_da are not implemented (the texture sampler differentiates the texture "
            "only): detach them")
MIP_FILTERS = ("linear-mipmap-nearest", "linear-mipmap-linear")


def _image(name: str, what: str, t: torch.Tensor, last: int):
    """([H,W,last] contiguous, had a minibatch axis)"""
    require_gpu(name, what, t, torch.float32, last)
    x, batched = ops._unbatch(name, what, t.detach(), 3)
    return x.contiguous(), batched


@torch.no_grad()
def rast_derivatives(rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor) -> torch.Tensor:
    """``rast_db`` float32 [H,W,4] = (du/dX, du/dY, dv/dX, dv/dY) per pixel step of the unsnapped (u, v) of include/gd_mesh.h,
    zeros on background: the second output of ``dr.rasterize``.  ``rast``: what ``mesh_render.rasterize(pos, tri, ...)``
    returned.  Not differentiable."""
    r, batched = _image("rast_derivatives", "rast", rast, 4)
    require_gpu("rast_derivatives", "pos", pos, torch.float32, 4)
    require_gpu("rast_derivatives", "tri", tri, torch.int32, 3)
    p = ops._unbatch("rast_derivatives", "pos", pos.detach(), 2)[0].contiguous()
    if tri.dim() != 2:
        raise ValueError("rast_derivatives: tri must be [F,3]")
    H, W = r.shape[:2]
    out = torch.empty((H, W, 4), dtype=torch.float32, device=r.device)
    launch("gd_sample_rast_db", r.device, p.shape[0], tri.shape[0], H, W, r, p, tri.contiguous(), out)
    return out[None] if batched else out


@torch.no_grad()
def interpolate_derivatives(attr: torch.Tensor, rast: torch.Tensor, rast_db: torch.Tensor, tri: torch.Tensor) -> torch.Tensor:
    """float32 [H,W,2C]: element 2k is d attr_k / dX and 2k + 1 is d attr_k / dY of the interpolated ``attr`` (float32 [V,C],
    C <= 8), zeros on background: the second output of ``dr.interpolate(attr, rast, tri, rast_db=rast_db,
    diff_attrs='all')``.  Not differentiable."""
    require_gpu("interpolate_derivatives", "attr", attr, torch.float32)
    a = ops._unbatch("interpolate_derivatives", "attr", attr.detach(), 2)[0].contiguous()
    r, b1 = _image("interpolate_derivatives", "rast", rast, 4)
    db, b2 = _image("interpolate_derivatives", "rast_db", rast_db, 4)
    require_gpu("interpolate_derivatives", "tri", tri, torch.int32, 3)
    if not 1 <= a.shape[1] <= mr.MAX_CHANNELS:
        raise ValueError(f"interpolate_derivatives: attr must have 1..{mr.MAX_CHANNELS} channels")
    if tuple(db.shape) != tuple(r.shape) or tri.dim() != 2:
        raise ValueError("interpolate_derivatives: rast and rast_db must be [H,W,4] of one resolution and tri [F,3]")
    H, W = r.shape[:2]
    out = torch.empty((H, W, 2 * a.shape[1]), dtype=torch.float32, device=r.device)
    launch("gd_sample_interpolate_da", r.device, a.shape[0], tri.shape[0], a.shape[1], H, W, a, r, db, tri.contiguous(), out)
    return out[None] if (b1 or b2) else out


# ---- the pyramid ------------------------------------------------------------------------------------------------------

class Mipmaps(NamedTuple):
    buffer: torch.Tensor                 # float32 [texels, 4]: every level, texels padded to 16 bytes (include/gd_sample.h)
    layout: _native.SamplePyramid        # levels, their sides and their offsets in texels
    source: torch.Tensor                 # float32 [H,W,C]: what the pyramid was built from; the gradient goes here
    shapes: Tuple[Tuple[int, int], ...]  # (Hl, Wl) per level
    offsets: Tuple[int, ...]             # first texel of each level, then the total


def pyramid_layout(height: int, width: int, max_mip_level: Optional[int]) -> _native.SamplePyramid:
    """The layout of include/gd_sample.h for a texture of ``height`` x ``width``; ``None``: down to 1 x 1"""
    layout = _native.SamplePyramid()
    level = -1 if max_mip_level is None else int(max_mip_level)
    if max_mip_level is not None and level < 0:
        raise ValueError("build_mipmaps: max_mip_level must be None or at least 0")
    _native.checked("gd_sample_pyramid_layout",
                    _native.lib().gd_sample_pyramid_layout(int(height), int(width), level, ctypes.byref(layout)))
    return layout


def _texture_image(name: str, tex: torch.Tensor) -> torch.Tensor:
    """float32 [H,W,C] of a float32 or uint8 (``u8 / 255``) texture, [H,W,C] or [1,H,W,C]; a float32 one keeps its graph"""
    require_gpu(name, "tex", tex)
    t = ops._unbatch(name, "tex", tex, 3)[0]
    if t.dtype == torch.uint8:
        # a tensor divisor: torch turns a division by a Python scalar into a product with its reciprocal
        t = t.to(torch.float32) / torch.full((), 255.0, dtype=torch.float32, device=t.device)
    elif t.dtype != torch.float32:
        raise TypeError(f"{name}: tex must be float32 or uint8")
    if not 1 <= t.shape[2] <= _native.SAMPLE_MAX_CHANNELS:
        raise ValueError(f"{name}: tex must have 1..{_native.SAMPLE_MAX_CHANNELS} channels")
    return t


def build_mipmaps(tex: torch.Tensor, max_mip_level: Optional[int] = None) -> Mipmaps:
    """The mip pyramid of ``tex`` (float32 [H,W,C], or uint8 converted as ``u8 / 255``; C <= 4): level ``l`` is
    ``max(W >> l, 1)`` wide, each texel the mean of its 2 x 2 parents, down to 1 x 1 or ``max_mip_level``.  More than one
    level needs power-of-two sides (``max_mip_level=0`` takes any).  Pass the result as ``texture(..., mip=)`` to build it
    once for many calls; the gradient of those calls goes to ``tex``."""
    t = _texture_image("build_mipmaps", tex)
    H, W, C = t.shape
    layout = pyramid_layout(H, W, max_mip_level)
    n = layout.levels
    buffer = torch.empty((layout.offset[n], _native.SAMPLE_TEXEL), dtype=torch.float32, device=t.device)
    launch("gd_sample_build_mips", t.device, C, t.detach().contiguous(), layout, buffer)
    return Mipmaps(buffer, layout, t, tuple((layout.height[l], layout.width[l]) for l in range(n)),
                   tuple(layout.offset[l] for l in range(n + 1)))


# ---- sampling ---------------------------------------------------------------------------------------------------------

def texture_backward(layout, channels: int, uv: torch.Tensor, uv_da: Optional[torch.Tensor], dout: torch.Tensor,
                     filter_id: int, boundary_id: int, dtex: torch.Tensor) -> torch.Tensor:
    """ADD the gradient of ``texture`` with respect to the texture to ``dtex`` (float32 [H,W,C], contiguous) and return it:
    steps 1-4 of include/gd_sample.h.  ``uv`` [N,2], ``uv_da`` [N,4] or None, ``dout`` [N,C], all contiguous float32.  The
    stable sort is ``torch.sort``; nothing is read back."""
    dev, N = uv.device, uv.shape[0]
    taps = _native.lib().gd_sample_taps(filter_id)
    keys = torch.empty(N * taps, dtype=torch.int64, device=dev)
    vals = torch.empty((N * taps, channels), dtype=torch.float32, device=dev)
    launch("gd_sample_texture_items", dev, N, channels, filter_id, boundary_id, layout, uv, uv_da, dout, keys, vals)
    skeys, order = torch.sort(keys, stable=True)
    gpyr = torch.zeros((layout.offset[layout.levels], _native.SAMPLE_TEXEL), dtype=torch.float32, device=dev)
    launch("gd_sample_texture_reduce", dev, N * taps, channels, layout, skeys, order, vals, gpyr)
    launch("gd_sample_texture_fold", dev, channels, layout, gpyr, dtex)
    return dtex


class _Texture(torch.autograd.Function):
    """``out`` [N,C] of the pyramid ``buffer``; the gradient goes to ``source``, the texture the pyramid was built from"""

    @staticmethod
    def forward(ctx, source, buffer, layout, uv, uv_da, filter_id, boundary_id):
        C, N = source.shape[2], uv.shape[0]
        out = torch.empty((N, C), dtype=torch.float32, device=uv.device)
        launch("gd_sample_texture_forward", uv.device, N, C, filter_id, boundary_id, layout, buffer, uv, uv_da, out)
        ctx.save_for_backward(uv, uv_da)
        ctx.args = (layout, tuple(source.shape), filter_id, boundary_id)
        return out

    @staticmethod
    def backward(ctx, dout):
        uv, uv_da = ctx.saved_tensors
        layout, shape, filter_id, boundary_id = ctx.args
        dtex = None
        if ctx.needs_input_grad[0]:
            dtex = torch.zeros(shape, dtype=torch.float32, device=uv.device)
            texture_backward(layout, shape[2], uv, uv_da, dout.contiguous(), filter_id, boundary_id, dtex)
        return dtex, None, None, None, None, None, None


def texture(tex: Optional[torch.Tensor], uv: torch.Tensor, uv_da: Optional[torch.Tensor] = None,
            mip: Optional[Mipmaps] = None, filter_mode: str = "auto", boundary_mode: str = "wrap",
            max_mip_level: Optional[int] = None) -> torch.Tensor:
    """``dr.texture``: sample ``tex`` (float32 or uint8 [Ht,Wt,C], C <= 4; row 0 is ``v = 0``, texel centres at
    ``(i + 0.5) / Wt``) at ``uv`` [...,2]; returns float32 [...,C].  ``filter_mode``: ``nearest``, ``linear``,
    ``linear-mipmap-nearest``, ``linear-mipmap-linear`` or ``auto`` (``linear-mipmap-linear`` when ``uv_da`` is given, else
    ``linear``); the mip filters need ``uv_da`` [...,4] = (du/dX, du/dY, dv/dX, dv/dY) (``interpolate_derivatives`` of the
    uv attributes) and power-of-two sides.  ``boundary_mode``: ``wrap`` (what the reference's call gets) or ``clamp`` (what
    an atlas wants).  ``mip``: a pyramid of ``build_mipmaps``, used instead of ``tex`` (which may then be ``None``);
    otherwise one is built here, down to ``max_mip_level``.  A pixel with a non-finite u or v gives zeros.

    Differentiable in the texture only (the gradient goes to ``tex``, or to the tensor ``mip`` was built from): every
    contribution is written once, sorted stably by destination and summed in a fixed order, so the gradient is
    bit-reproducible.  ``uv`` or ``uv_da`` requiring a gradient raises ``NotImplementedError``."""
    require_gpu("texture", "uv", uv, torch.float32, 2)
    if filter_mode == "auto":
        filter_mode = "linear-mipmap-linear" if uv_da is not None else "linear"
    if filter_mode not in _native.SAMPLE_FILTERS:
        raise ValueError(f"texture: filter_mode must be 'auto' or one of {sorted(_native.SAMPLE_FILTERS)}, not {filter_mode!r}")
    if boundary_mode not in _native.SAMPLE_BOUNDARIES:
        raise ValueError(f"texture: boundary_mode must be one of {sorted(_native.SAMPLE_BOUNDARIES)}, not {boundary_mode!r} "
                         "('cube' and 'zero' are not built)")
    mipped = filter_mode in MIP_FILTERS
    if mipped and uv_da is None:
        raise ValueError(f"texture: filter_mode {filter_mode!r} needs uv_da")
    grad = torch.is_grad_enabled()
    if grad and (uv.requires_grad or (uv_da is not None and uv_da.requires_grad)):
        raise NotImplementedError("texture: " + _UV_GRAD)
    da = None
    if uv_da is not None and mipped:
        require_gpu("texture", "uv_da", uv_da, torch.float32, 4)
        if tuple(uv_da.shape[:-1]) != tuple(uv.shape[:-1]):
            raise ValueError("texture: uv_da must be [...,4] with the leading shape of uv")
        da = uv_da.detach().reshape(-1, 4).contiguous()
    if mip is None:
        if tex is None:
            raise ValueError("texture: give tex or mip")
        mip = build_mipmaps(tex, max_mip_level if mipped else 0)
    elif not isinstance(mip, Mipmaps):
        raise TypeError("texture: mip must be the Mipmaps of build_mipmaps")
    if mip.buffer.device != uv.device:
        raise ValueError("texture: the texture and uv must be on one device")
    flat = uv.detach().reshape(-1, 2).contiguous()
    if flat.shape[0] == 0:
        raise ValueError("texture: uv holds no pixel")
    out = _Texture.apply(mip.source, mip.buffer, mip.layout, flat, da, _native.SAMPLE_FILTERS[filter_mode],
                         _native.SAMPLE_BOUNDARIES[boundary_mode])
    return out.view(*uv.shape[:-1], mip.source.shape[2])


# ---- the textured render ----------------------------------------------------------------------------------------------

def _vertex_normals(v: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    from . import mesh_geometry as mg
    return mg.normals(v, mg.build_geometry(f, num_vertices=v.shape[0], device=v.device))[1].detach()


def clip_positions(v: torch.Tensor, pose, proj):
    """(v_cam [V,4], v_clip [V,4], pose as a device tensor) of ``v`` [V,3] under ``pose`` / ``proj`` (numpy [4,4]), as
    ``render_mesh`` forms them (``torch.inverse`` waits for the GPU)"""
    pose_t = torch.from_numpy(np.asarray(pose).astype(np.float32)).to(v.device)
    proj_t = torch.from_numpy(np.asarray(proj).astype(np.float32)).to(v.device)
    v_cam = torch.matmul(torch.nn.functional.pad(v, pad=(0, 1), mode="constant", value=1.0), torch.inverse(pose_t).T).float()
    return v_cam, (v_cam @ proj_t.T).contiguous(), pose_t


def render_mesh(v: torch.Tensor, f: torch.Tensor, vt, ft, albedo, vn, pose, proj, h: int, w: int, bg_color=1,
                texture_filter: str = "linear-mipmap-linear", boundary_mode: str = "wrap", vc: Optional[torch.Tensor] = None,
                ssaa: int = 1) -> dict:
    """The reference's ``render_mesh`` (mesh_renderer.py:42-101) for ``ssaa = 1``: rasterize, interpolate ``vt`` over ``ft``
    with its screen-space derivatives, sample ``albedo`` (a texture of ``texture``, or the ``Mipmaps`` of one) with
    ``texture_filter`` / ``boundary_mode``, antialias, composite over ``bg_color``.  ``vc`` (float32 [V,3]) replaces the
    texture by interpolated vertex colours.  ``v`` float32 [V,3], ``f`` int [F,3], ``vt`` float32 [T,2] in the package's
    atlas convention (row 0 of ``albedo`` is ``v = 0``; ``load_textured_obj`` returns it so), ``ft`` int [F,3], ``vn``
    float32 [V,3] or ``None``, ``pose`` (camera to world) and ``proj`` numpy [4,4].

    Returns the reference's dict: ``image`` [H,W,3] clamped to [0,1], ``alpha`` [H,W,1], ``depth`` [H,W,1], ``normal``
    [H,W,3] in [0,1], ``viewcos`` [H,W,1].  Two departures from the reference's function, both towards its own
    ``Renderer.render`` and this package's ``MeshRenderer.render``, with which ``alpha``, ``depth`` and ``normal`` agree:
    ``alpha`` is the antialiased coverage (the reference's ``render_mesh`` keeps the hard mask ``rast > 0``), and one
    silhouette analysis serves alpha and colour.  With ``vn=None`` the normals are ``mesh_geometry.normals``: the
    normalised sum of the unit face normals with ``F.normalize``'s 1e-12, where the reference leaves the SUM of unit face
    normals unnormalised and replaces a sum below 1e-20 by (0, 0, 1) -- after interpolation and ``safe_normalize`` the two
    differ inside a triangle whose corners' sums have different lengths, and at a vertex no face uses (0 here).
    ``ssaa != 1`` raises (kiui's ``scale_img_hwc`` is not restated here).  The gradient reaches ``albedo`` only."""
    if ssaa != 1:
        raise ValueError("render_mesh: ssaa != 1 is not implemented")
    require_gpu("render_mesh", "v", v, torch.float32, 3)
    require_gpu("render_mesh", "f", f)
    dev = v.device
    h, w = int(h), int(w)
    v = v.detach().contiguous()
    f = f.detach().to(torch.int32).contiguous()
    v_cam, v_clip, pose_t = clip_positions(v, pose, proj)
    topo = mr.build_topology(f, num_vertices=v.shape[0], device=dev)

    rast = mr.rasterize(v_clip, f, (h, w))
    wts = mr.antialias_weights(rast, v_clip, f, topo)
    alpha = torch.clamp(rast[..., -1:], 0, 1).contiguous()
    alpha = mr.antialias(alpha, rast, v_clip, f, weights=wts).clamp(0, 1)
    depth = mr.interpolate(-v_cam[..., 2:3].contiguous(), rast, f)

    if vc is not None:
        require_gpu("render_mesh", "vc", vc, torch.float32, 3)
        color = mr.interpolate(vc.detach().contiguous(), rast, f)
    else:
        vt = torch.as_tensor(np.asarray(vt) if not isinstance(vt, torch.Tensor) else vt).to(dev, torch.float32).contiguous()
        ft = torch.as_tensor(np.asarray(ft) if not isinstance(ft, torch.Tensor) else ft).to(dev, torch.int32).contiguous()
        if tuple(ft.shape) != tuple(f.shape):
            raise ValueError("render_mesh: ft must have one row per face of f")
        texc = mr.interpolate(vt, rast, ft)
        texc_da = None
        if texture_filter in MIP_FILTERS:
            texc_da = interpolate_derivatives(vt, rast, rast_derivatives(rast, v_clip, f), ft)
        if isinstance(albedo, Mipmaps):
            color = texture(None, texc, texc_da, mip=albedo, filter_mode=texture_filter, boundary_mode=boundary_mode)
        else:
            color = texture(albedo, texc, texc_da, filter_mode=texture_filter, boundary_mode=boundary_mode)
        if color.shape[-1] != 3:
            raise ValueError("render_mesh: albedo must have 3 channels")
    color = mr.antialias(color, rast, v_clip, f, weights=wts)
    color = alpha * color + (1 - alpha) * bg_color

    if vn is None:
        vn = _vertex_normals(v, f)
    require_gpu("render_mesh", "vn", vn, torch.float32, 3)
    normal = mr.safe_normalize(mr.interpolate(vn.detach().contiguous(), rast, f))
    viewcos = (normal @ pose_t[:3, :3])[..., 2:3]
    return {"image": color.clamp(0, 1), "alpha": alpha, "depth": depth, "normal": (normal + 1) / 2, "viewcos": viewcos}


def load_textured_obj(path: str):
    """``(v float64 [V,3], f int64 [F,3], vt float64 [T,2], ft int64 [F,3], albedo uint8 [H,W,3 or 4])`` (numpy) of a
    textured ``.obj``: ``template.load_obj_uv`` and the ``map_Kd`` image of its ``mtllib`` (``export.load_image_rgb``).
    ``vt`` is returned in the package's atlas convention: the ``1 - v`` that ``write_textured_obj`` writes is undone, so
    that ``v = 0`` is the PNG's first row."""
    v, f, vt, ft = load_obj_uv(path)
    if vt is None:
        raise ValueError(f"{path}: the faces carry no texture coordinates")
    folder = os.path.dirname(os.path.abspath(path))
    mtl = None
    with open(path, "r") as src:
        for line in src:
            tok = line.split("#", 1)[0].split()
            if tok and tok[0] == "mtllib" and len(tok) > 1:
                mtl = os.path.join(folder, line.split("#", 1)[0].split(None, 1)[1].strip())
                break
    if mtl is None:
        raise ValueError(f"{path}: no mtllib line")
    image = None
    with open(mtl, "r") as src:
        for line in src:
            tok = line.split("#", 1)[0].split()
            if tok and tok[0] == "map_Kd" and len(tok) > 1:
                image = os.path.join(os.path.dirname(mtl), tok[-1])
                break
    if image is None:
        raise ValueError(f"{mtl}: no map_Kd line")
    vt = vt.copy()
    vt[:, 1] = 1.0 - vt[:, 1]
    return v, f, vt, ft, load_image_rgb(image)
