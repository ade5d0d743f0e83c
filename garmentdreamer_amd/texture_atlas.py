"""A chart-based UV atlas for the textured-mesh export, the place of xatlas in the reference's ``mesh.auto_uv``
(Garment_Deformer_NeTF/netf/render/mesh_renderer.py:267), on the HIP kernels of ``csrc/raster_atlas.hip`` (C-ABI and the
definitions: include/gd_atlas.h) -- no CPU path, and a different algorithm from xatlas: a normal-bucketed orthographic
unwrap.

  * ``chart_atlas(vertices, indices, resolution=2048, gutter=2, max_rounds=8)``   ``(vt, ft, info)``
  * ``face_classes`` / ``chart_labels`` / ``chart_bounds``                         its stages, for callers and tests
  * ``pack_charts(bounds, resolution, gutter)``                                    the shelf packer (host, numpy, integers)

Every face is classed by the dominant axis and sign of its normal; a chart is a connected component of faces of one class
(and one layer); a chart is projected along its axis, all charts at one scale, and its bounding rectangle is shelf-packed.
A chart that overlaps itself in projection is peeled: the atlas is rasterized, the faces that lose a texel centre to
another face move to the next layer and the unwrap is repeated; after ``max_rounds`` such faces become charts of their own.

What is torch here is plumbing: allocation, ``torch.unique`` of the packed 64-bit (chart, vertex) keys, and the read-backs:
one flag per component sweep, one read of the chart count and one of the bounds per round (the packer runs on the host),
one of the lost count per round.  An unwrap happens once per run."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _native
from ._launch import launch
from .mesh_connectivity import Connectivity, build_connectivity, empty_i32, mesh_args, scan
from .mesh_render import rasterize

NAME = "texture_atlas"
_MESH = "mesh_remesh."   # the prefix the mesh checks' messages carry here: they were the remesher's own when this was written


# ---- the packer: include/gd_atlas.h "PACKING", line for line ---------------------------------------------------------------

def _rectangles(bounds: np.ndarray, s: np.float32, gutter: int) -> Tuple[np.ndarray, np.ndarray]:
    f256 = np.float32(256.0)
    ma = np.rint(((bounds[:, 2] - bounds[:, 0]) * s) * f256).astype(np.int64)
    mb = np.rint(((bounds[:, 3] - bounds[:, 1]) * s) * f256).astype(np.int64)
    return np.maximum((ma + 255) // 256, 1) + 2 * gutter, np.maximum((mb + 255) // 256, 1) + 2 * gutter


def _shelves(w: np.ndarray, h: np.ndarray, resolution: int) -> Optional[np.ndarray]:
    """int32 [C,2] offsets, or None if the rectangles do not fit"""
    order = np.lexsort((np.arange(w.shape[0]), -w, -h))
    out = np.zeros((w.shape[0], 2), dtype=np.int32)
    x = y = shelf = 0
    fresh = True
    for c, cw, ch in zip(order.tolist(), w[order].tolist(), h[order].tolist()):
        if cw > resolution:
            return None
        if x + cw > resolution:
            y, x, fresh = y + shelf, 0, True
        if fresh:
            shelf, fresh = ch, False
        if y + ch > resolution:
            return None
        out[c] = (x, y)
        x += cw
    return out


def pack_charts(bounds, resolution: int, gutter: int) -> Tuple[np.float32, np.ndarray, np.ndarray]:
    """``(scale float32, offsets int32 [C,2], sizes int32 [C,2])`` for ``bounds`` float32 [C,4] = (a_min, b_min, a_max,
    b_max): one scale for all charts, rectangles of whole texels with ``gutter`` on every side, shelf-packed into
    ``resolution``^2 in the order (height, width descending, chart ascending); the scale is what a bisection of
    ``ATLAS_BISECTION_STEPS`` steps finds.  ``ValueError`` if the charts' gutters alone do not fit."""
    bounds = np.ascontiguousarray(bounds, dtype=np.float32).reshape(-1, 4)
    res, g = int(resolution), int(gutter)
    with np.errstate(over="ignore", invalid="ignore"):
        def fit(s):
            w, h = _rectangles(bounds, np.float32(s), g)
            off = _shelves(w, h, res)
            return None if off is None else (np.float32(s), off, np.stack((w, h), axis=1).astype(np.int32))

        small = ValueError(f"chart_atlas: resolution {res} is too small for {bounds.shape[0]} charts with a gutter of {g}")
        if fit(0.0) is None:
            raise small
        d = bounds.astype(np.float64)
        d = float(max((d[:, 2] - d[:, 0]).max(), (d[:, 3] - d[:, 1]).max()))
        if not d > 0.0 or not np.isfinite(d):
            raise ValueError("chart_atlas: the charts have no extent")
        hi = (res - 2 * g) / d
        best = fit(np.float32(hi))
        if best is not None:
            return best
        lo = 0.0
        for _ in range(_native.ATLAS_BISECTION_STEPS):
            mid = float(np.float32((lo + hi) / 2))
            got = fit(mid)
            if got is not None:
                lo, best = mid, got
            else:
                hi = mid
        if best is None or not best[0] > 0:
            raise small
        return best


# ---- the stages ------------------------------------------------------------------------------------------------------------

def face_classes(vertices: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
    """int32 [F]: ``2 k + (n_k < 0)`` of the dominant axis ``k`` of each face's normal, 6 for a degenerate face."""
    v, t = mesh_args(_MESH + "face_classes", vertices, indices)
    cls = empty_i32(t.shape[0], v.device)
    launch("gd_atlas_face_class", v.device, v.shape[0], t.shape[0], v, t, cls)
    return cls


def chart_labels(conn: Connectivity, cls: torch.Tensor, layer: Optional[torch.Tensor] = None,
                 single: Optional[torch.Tensor] = None, return_sweeps: bool = False):
    """int32 [F]: per face the lowest face index of its chart (faces joined across interior edges where class and layer
    agree; a degenerate or ``single`` face is alone).  One host read per sweep; ``RuntimeError`` after
    ``ATLAS_MAX_SWEEPS`` sweeps that still changed something."""
    dev, F = cls.device, conn.F
    layer = torch.zeros(F, dtype=torch.int32, device=dev) if layer is None else layer
    single = torch.zeros(F, dtype=torch.int32, device=dev) if single is None else single
    parent = torch.arange(F, dtype=torch.int32, device=dev)
    changed = torch.zeros(_native.ATLAS_MAX_SWEEPS, dtype=torch.int32, device=dev)
    for sweep in range(_native.ATLAS_MAX_SWEEPS):
        launch("gd_atlas_hook", dev, F, conn.E, conn.eh, cls, layer, single, parent, changed[sweep:])
        launch("gd_atlas_jump", dev, F, parent)
        if not int(changed[sweep]):
            return (parent, sweep + 1) if return_sweeps else parent
    raise RuntimeError(f"{NAME}.chart_labels: the components still changed after {_native.ATLAS_MAX_SWEEPS} sweeps")


def chart_bounds(v: torch.Tensor, t: torch.Tensor, cls: torch.Tensor, labels: torch.Tensor):
    """``(C, face_chart int32 [F], bounds float32 [C,4], count int32 [C])``: charts numbered by ascending label"""
    dev, F = v.device, t.shape[0]
    is_root = empty_i32(F, dev)
    launch("gd_atlas_roots", dev, F, cls, labels, is_root)
    root_scan = scan(is_root)
    C = int(root_scan[-1])                                                # the chart count sizes the tables
    if C == 0:
        raise ValueError(f"{NAME}: every face is degenerate")
    face_chart, count = empty_i32(F, dev), empty_i32(C, dev)
    keys = torch.empty((C, 4), dtype=torch.int32, device=dev)
    bounds = torch.empty((C, 4), dtype=torch.float32, device=dev)
    launch("gd_atlas_bounds", dev, v.shape[0], F, C, v, t, cls, labels, root_scan, face_chart, keys, bounds, count)
    return C, face_chart, bounds, count


def _emit(v, t, cls, face_chart, bounds, C, resolution, gutter, scale, offsets):
    """(corner_xy int32 [F,3,2], vt float32 [T,2], ft int32 [F,3])"""
    dev, F = v.device, t.shape[0]
    corner_xy = torch.empty((F, 3, 2), dtype=torch.int32, device=dev)
    key = torch.empty(3 * F, dtype=torch.int64, device=dev)
    off = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.int32)).to(dev)
    launch("gd_atlas_emit", dev, v.shape[0], F, C, resolution, gutter, float(scale), v, t, cls, face_chart, bounds, off,
           corner_xy, key)
    rows, inverse = torch.unique(key, sorted=True, return_inverse=True)
    T = rows.shape[0]
    vt = torch.empty((T, 2), dtype=torch.float32, device=dev)
    ft = torch.empty((F, 3), dtype=torch.int32, device=dev)
    launch("gd_atlas_write_vt", dev, 3 * F, T, resolution, inverse.contiguous(), corner_xy, vt, ft)
    return corner_xy, vt, ft


def _rasterize_atlas(vt: torch.Tensor, ft: torch.Tensor, resolution: int) -> torch.Tensor:
    pos = torch.cat((vt * 2.0 - 1.0, torch.zeros_like(vt[:, :1]), torch.ones_like(vt[:, :1])), dim=1).contiguous()
    return rasterize(pos, ft, (resolution, resolution))


@torch.no_grad()
def chart_atlas(vertices: torch.Tensor, indices: torch.Tensor, resolution: int = 2048, gutter: int = 2,
                max_rounds: int = 8, trace: Optional[List[Dict]] = None) -> Tuple[torch.Tensor, torch.Tensor, Dict]:
    """``(vt float32 [T,2], ft int32 [F,3], info)`` on the device of ``vertices`` (float32 [V,3]; ``indices`` int32 or int64
    [F,3]).  ``vt`` has one row per (chart, vertex) pair, so the faces of a chart share rows and different charts never do;
    every corner lies on the 1/256-texel grid of ``resolution``, where the rasterizer snaps it anyway.  ``info``:
    ``num_charts``, ``face_chart`` (int32 [F] on the device, -1 for a degenerate face), ``scale`` (texels per unit length),
    ``rounds`` and ``lost_per_round`` of the overlap peeling, ``singletons``, ``seam_edges`` (interior edges between two
    charts) and ``coverage`` (the fraction of texel centres covered).  A face still lost after ``max_rounds`` rounds becomes
    a chart of its own, and further rounds do only that until a round loses nothing.  ``trace``: a list that receives
    each round's tensors (tests).  ``ValueError`` for a non-manifold mesh and for a resolution too small for the charts'
    gutters."""
    v, t = mesh_args(_MESH + "chart_atlas", vertices, indices)
    res, g, max_rounds = int(resolution), int(gutter), int(max_rounds)
    if not 1 <= res <= _native.ATLAS_MAX_RESOLUTION or not 0 <= g <= _native.ATLAS_MAX_GUTTER or max_rounds < 1:
        raise ValueError(f"chart_atlas: resolution must be in 1..{_native.ATLAS_MAX_RESOLUTION}, gutter in "
                         f"0..{_native.ATLAS_MAX_GUTTER} and max_rounds at least 1")
    if t.shape[0] == 0:
        raise ValueError("chart_atlas: the mesh has no faces")
    dev, F = v.device, t.shape[0]
    conn = build_connectivity(t, v.shape[0], _MESH + "chart_atlas")
    cls = face_classes(v, t)
    layer = torch.zeros(F, dtype=torch.int32, device=dev)
    single = torch.zeros(F, dtype=torch.int32, device=dev)
    lost_per_round: List[int] = []
    while True:
        rnd = len(lost_per_round) + 1
        labels, sweeps = chart_labels(conn, cls, layer, single, return_sweeps=True)
        C, face_chart, bounds, count = chart_bounds(v, t, cls, labels)
        scale, offsets, sizes = pack_charts(bounds.cpu().numpy(), res, g)       # the one read of the bounds
        corner_xy, vt, ft = _emit(v, t, cls, face_chart, bounds, C, res, g, scale, offsets)
        rast = _rasterize_atlas(vt, ft, res)
        lost = empty_i32(F, dev)
        before = (layer.clone(), single.clone()) if trace is not None else None
        launch("gd_atlas_lost_faces", dev, F, res, res, corner_xy, rast, int(rnd >= max_rounds), lost, layer, single)
        n_lost = int(lost.sum())
        lost_per_round.append(n_lost)
        if trace is not None:
            trace.append({"layer": before[0], "single": before[1], "labels": labels, "sweeps": sweeps,
                          "face_chart": face_chart, "bounds": bounds, "count": count, "scale": scale, "offsets": offsets,
                          "sizes": sizes, "corner_xy": corner_xy, "vt": vt, "ft": ft, "lost": lost})
        if n_lost == 0:
            break
        if rnd >= max_rounds + F:                                       # every round past max_rounds adds a singleton
            raise RuntimeError("chart_atlas: the overlap peeling did not end")
    inner = conn.eh[:, 1] >= 0
    fa = face_chart[(conn.eh[:, 0] // 3).long()]
    fb = face_chart[(conn.eh[:, 1].clamp(min=0) // 3).long()]
    info = {"num_charts": C, "face_chart": face_chart, "scale": float(scale), "rounds": len(lost_per_round),
            "lost_per_round": lost_per_round, "singletons": int(single.sum()),
            "seam_edges": int((inner & (fa != fb)).sum()), "coverage": float((rast[..., 3] > 0).sum()) / float(res * res)}
    return vt, ft, info
