"""The way out of the NeTF stage: bake a trained ``TextureField`` into a UV atlas and write the textured mesh, the file
``Renderer.export_mesh`` leaves at the end of the reference's run
(Garment_Deformer_NeTF/netf/render/mesh_renderer.py:260-313), without xatlas, nvdiffrast or kiui.

  * ``grid_atlas(num_faces, resolution, gutter)``   an atlas that needs no unwrap: every triangle is its own right-triangle
                                                    chart, two per square cell (host, deterministic).  SEAM-HEAVY: every
                                                    edge of the mesh is a seam; the chart-based unwrap is
                                                    ``texture_atlas.chart_atlas`` (``atlas="chart"`` below)
  * ``uv_padding_index(mask, padding)``             per texel the covered texel it takes its colour from: the HIP kernel of
                                                    ``csrc/raster_bake.hip`` (definition: include/gd_bake.h) -- no CPU path
  * ``uv_padding(image, mask, padding)``            the padded 8-bit image (``gd_bake_resolve_u8`` after the index)
  * ``bake_texture(field, v, f, vt, ft, ...)``      rasterize the atlas, interpolate positions, query the field, pad
  * ``write_textured_obj(path, ...)``               ``.obj`` + ``.mtl`` + ``_albedo.png``
  * ``load_obj_uv(path)``                           ``template.load_obj_uv``: reads such a file back

Atlas row ``r`` holds ``v = (r + 0.5) / H``: row 0 is ``v = 0``, the rasterizer's convention (row 0 is ``y_ndc = -1``).  The
files are written for viewers with ``v`` up: ``vt`` lines carry ``1 - v`` and the PNG's first row is atlas row 0.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Tuple

import numpy as np
import torch

from ._launch import launch, require_gpu
from .export import save_image_rgb
from .mesh_render import interpolate, rasterize
from .template import load_obj_uv  # noqa: F401  (re-exported)


def grid_atlas(num_faces: int, resolution: int, gutter: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """(vt float32 [3F,2], ft int32 [F,3]).  ``n = ceil(sqrt(ceil(F / 2)))`` cells per side of ``s = resolution // n``
    texels; triangles ``2k`` and ``2k + 1`` share the cell at column ``k % n``, row ``k // n``, origin (cx, cy) = (s col,
    s row).  With ``g = gutter`` and leg ``l = s - 3 g``:

        even t:  (cx + g, cy + g), (cx + g + l, cy + g), (cx + g, cy + g + l)
        odd t:   (cx + s - g, cy + s - g), (cx + s - g - l, cy + s - g), (cx + s - g, cy + s - g - l)

    in texels, ``vt = texel / resolution``.  The two hypotenuses of a cell are ``sqrt(2) g`` apart and every chart keeps
    ``g`` texels from its cell's border, so no two charts overlap.  ``ValueError`` if ``l < 1``."""
    F, res, g = int(num_faces), int(resolution), int(gutter)
    if F < 1 or res < 1 or g < 0:
        raise ValueError("grid_atlas: num_faces and resolution must be at least 1, gutter at least 0")
    pairs = (F + 1) // 2
    n = math.isqrt(pairs - 1) + 1                      # ceil(sqrt(pairs)) in integers
    s = res // n
    leg = s - 3 * g
    if leg < 1:
        raise ValueError(f"grid_atlas: {F} faces at resolution {res} leave cells of {s} texels, too small for a gutter "
                         f"of {g} (the chart's leg would be {leg})")
    t = np.arange(F, dtype=np.int64)
    k = t // 2
    cx, cy = s * (k % n), s * (k // n)
    odd = (t % 2 == 1)
    x0 = np.where(odd, cx + s - g, cx + g)
    y0 = np.where(odd, cy + s - g, cy + g)
    step = np.where(odd, -leg, leg)
    texel = np.stack((np.stack((x0, y0), axis=1), np.stack((x0 + step, y0), axis=1), np.stack((x0, y0 + step), axis=1)),
                     axis=1)                           # [F, 3 corners, 2]
    vt = (texel.reshape(-1, 2).astype(np.float64) / res).astype(np.float32)
    return vt, np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def _mask_u8(name: str, mask) -> torch.Tensor:
    require_gpu(name, "mask", mask)
    if mask.dim() != 2:
        raise ValueError(f"{name}: mask must be [H,W]")
    if mask.dtype == torch.bool:
        mask = mask.contiguous().view(torch.uint8)     # same bytes: True is 1
    elif mask.dtype != torch.uint8:
        raise TypeError(f"{name}: mask must be bool or uint8")
    return mask.contiguous()


def uv_padding_index(mask: torch.Tensor, padding: int) -> torch.Tensor:
    """``src`` int32 [H,W] of include/gd_bake.h: a covered texel's own row-major index; for an uncovered texel with a
    covered one within L1 distance ``padding`` the nearest covered texel (squared Euclidean distance, lowest index among
    equals); -1 elsewhere.  ``mask``: bool or uint8 [H,W] on the GPU; ``0 <= padding <= 64``.  One launch, no host wait."""
    m = _mask_u8("uv_padding_index", mask)
    H, W = m.shape
    src = torch.empty((H, W), dtype=torch.int32, device=m.device)
    launch("gd_bake_pad_index", m.device, H, W, int(padding), m, src)
    return src


def resolve_u8(image: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """uint8 [H,W,C]: ``(uint8)(int)(clamp(image[src], 0, 1) * 255)`` where ``src >= 0``, 0 elsewhere (NaN gives 0).
    ``image``: float32 [H,W,C], C <= 4; ``src``: int32 [H,W]."""
    require_gpu("resolve_u8", "image", image)
    require_gpu("resolve_u8", "src", src)
    if image.dtype != torch.float32 or src.dtype != torch.int32:
        raise TypeError("resolve_u8: image must be float32 and src int32")
    if image.dim() != 3 or src.dim() != 2 or tuple(image.shape[:2]) != tuple(src.shape) or image.device != src.device:
        raise ValueError("resolve_u8: image must be [H,W,C] and src [H,W] on one device")
    H, W, C = image.shape
    img, s = image.detach().contiguous(), src.contiguous()
    out = torch.empty((H, W, C), dtype=torch.uint8, device=img.device)
    launch("gd_bake_resolve_u8", img.device, H, W, C, img, s, out)
    return out


def uv_padding(image: torch.Tensor, mask: torch.Tensor, padding: int) -> torch.Tensor:
    """kiui's ``uv_padding(image, mask, padding)`` with the tie rule of include/gd_bake.h, quantised: uint8 [H,W,C] in which
    every texel within L1 distance ``padding`` of the mask holds its nearest covered texel's colour and the rest is 0."""
    require_gpu("uv_padding", "image", image)
    return resolve_u8(image, uv_padding_index(mask, padding))


@torch.no_grad()
def bake_texture(field, v: torch.Tensor, f: torch.Tensor, vt, ft, resolution: int = 2048, padding: int = 16) -> Dict:
    """Bake ``field`` (a ``TextureField``: ``field(xyz [N,3], mask uint8 [N]) -> [N,3]``) over the mesh ``v`` float32 [V,3] /
    ``f`` int [F,3] into the atlas ``vt`` [T,2] / ``ft`` [F,3] (arrays or tensors; face ``t`` of ``ft`` is face ``t`` of ``f``).
    Returns ``albedo`` uint8 [H,W,3], ``mask`` bool [H,W] (texels whose centre a chart covers) and ``src`` int32 [H,W], all
    on the device of ``v``.  The atlas is rasterized as the triangles (2u - 1, 2v - 1, 0, 1), positions are interpolated
    with the atlas's barycentrics over ``f``, the field is asked once for the whole atlas with the coverage as its mask,
    and the charts are padded by ``padding`` texels (``uv_padding``)."""
    require_gpu("bake_texture", "v", v)
    require_gpu("bake_texture", "f", f)
    dev = v.device
    H = W = int(resolution)
    vt = torch.as_tensor(np.asarray(vt) if not isinstance(vt, torch.Tensor) else vt).to(dev, torch.float32)
    ft = torch.as_tensor(np.asarray(ft) if not isinstance(ft, torch.Tensor) else ft).to(dev, torch.int32).contiguous()
    f = f.detach().to(torch.int32).contiguous()
    if vt.dim() != 2 or vt.shape[1] != 2 or ft.dim() != 2 or tuple(ft.shape) != tuple(f.shape):
        raise ValueError("bake_texture: vt must be [T,2] and ft [F,3], one row per face of f")
    pos = torch.cat((vt * 2.0 - 1.0, torch.zeros_like(vt[:, :1]), torch.ones_like(vt[:, :1])), dim=1).contiguous()
    rast = rasterize(pos, ft, (H, W))
    xyz = interpolate(v.detach().float().contiguous(), rast, f)
    mask = rast[..., 3] > 0
    color = field(xyz.view(-1, 3), mask.view(-1)).float().view(H, W, 3)
    src = uv_padding_index(mask, padding)
    return {"albedo": resolve_u8(color, src), "mask": mask, "src": src}


def _host(a, dtype) -> np.ndarray:
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dtype)


def write_textured_obj(path: str, v, f, vt, ft, albedo, reverse: bool = False) -> List[str]:
    """Write ``path`` (``mtllib``, ``v``, ``vt u (1 - v)``, ``usemtl``, ``f a/b`` with 1-based indices), ``<stem>.mtl`` (one
    material, ``map_Kd <stem>_albedo.png``) and ``<stem>_albedo.png`` (8-bit RGB, atlas row 0 first) next to it; returns
    the three paths.  ``albedo``: uint8 [H,W,3]; ``reverse`` negates x of the written vertices and leaves the faces alone,
    as the reference does."""
    v, vt = _host(v, np.float64).reshape(-1, 3).copy(), _host(vt, np.float64).reshape(-1, 2)
    f, ft = _host(f, np.int64).reshape(-1, 3), _host(ft, np.int64).reshape(-1, 3)
    if f.shape != ft.shape:
        raise ValueError("write_textured_obj: f and ft must have one row per face")
    if reverse:
        v[:, 0] = -v[:, 0]
    folder = os.path.dirname(os.path.abspath(path))
    stem = os.path.splitext(os.path.basename(path))[0]
    mtl_path = os.path.join(folder, stem + ".mtl")
    png_path = os.path.join(folder, stem + "_albedo.png")
    os.makedirs(folder, exist_ok=True)
    save_image_rgb(png_path, albedo)
    lines = [f"mtllib {stem}.mtl"]
    lines += ["v %r %r %r" % (float(x), float(y), float(z)) for x, y, z in v]
    lines += ["vt %r %r" % (float(a), 1.0 - float(b)) for a, b in vt]
    lines.append("usemtl defaultMat")
    lines += ["f %d/%d %d/%d %d/%d" % (a[0] + 1, b[0] + 1, a[1] + 1, b[1] + 1, a[2] + 1, b[2] + 1) for a, b in zip(f, ft)]
    with open(path, "w") as out:
        out.write("\n".join(lines) + "\n")
    with open(mtl_path, "w") as out:
        out.write("newmtl defaultMat\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nTr 1\nillum 1\nNs 0\n"
                  f"map_Kd {stem}_albedo.png\n")
    return [path, mtl_path, png_path]


def export_textured_mesh(save_path: str, field, v: torch.Tensor, f: torch.Tensor, texture_resolution: int = 2048,
                         padding: int = 16, reverse: bool = False, vt=None, ft=None, atlas: str = "grid") -> List[str]:
    """``bake_texture`` + ``write_textured_obj``: the body of ``NeTFRenderer.export_mesh``.  Without ``vt`` / ``ft`` the
    atlas is ``grid_atlas(F, texture_resolution)`` for ``atlas="grid"`` and ``texture_atlas.chart_atlas(v, f,
    texture_resolution)`` for ``atlas="chart"``; UVs given by the caller win."""
    if (vt is None) != (ft is None):
        raise ValueError("export_mesh: give both vt and ft, or neither")
    if atlas not in ("grid", "chart"):
        raise ValueError(f"export_mesh: atlas must be 'grid' or 'chart', not {atlas!r}")
    if vt is None and atlas == "chart":
        from .texture_atlas import chart_atlas
        vt, ft, _ = chart_atlas(v, f, texture_resolution)
    elif vt is None:
        vt, ft = grid_atlas(f.shape[0], texture_resolution)
    baked = bake_texture(field, v, f, vt, ft, texture_resolution, padding)
    return write_textured_obj(save_path, v, f, vt, ft, baked["albedo"], reverse=reverse)
