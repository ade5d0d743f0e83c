"""Isotropic remeshing of the deformer's mesh on the GPU: the place of ``gpytoolbox.remesh_botsch`` in the reference's
upsample iterations (``Garment_Deformer_NeTF/deformation.py:273-295``), on the HIP kernels of ``csrc/raster_remesh.hip``
(C-ABI and definitions: include/gd_mesh_remesh.h) -- no CPU path.

  * ``remesh_botsch(vertices, indices, h, iterations=10, project=True, rounds=4)``   the whole remesh:
        ``iterations`` x (split -> collapse rounds -> flip rounds -> relax -> project)
  * ``split_long_edges`` / ``collapse_short_edges_round`` / ``flip_edges_round`` / ``tangential_relax`` /
    ``project_to_surface``                                   the single passes, for callers with a schedule of their own
  * ``mean_edge_length(vertices, geo)``                      of a ``mesh_geometry.MeshGeometry``, on the device

What is torch here is plumbing: allocation, ``torch.sort`` of the packed 64-bit keys, the copy of the old vertex rows, and
the read-back of counts that size the next buffer (a remesh happens once or twice per deformation).  Everything that derives
a table from sorted keys, decides or moves anything is a kernel.  Host reads: one per connectivity build (the edge count and
the input's error flags), two per split (new vertices and faces; the apply's flags), one or two per collapse round, one per
flip round (what it applied), one per projection (the unprojected count), one or two per vertex compaction: about 30 in an
iteration with full rounds.  The connectivity itself (``Connectivity``, ``build_connectivity``) lives in
``mesh_connectivity``, with the atlas and the final-mesh post-process as its other users; both names are re-exported here."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _native
from ._launch import launch, require_gpu
from .mesh_connectivity import (Connectivity, build_connectivity, drop_dead_faces, empty_i32, mesh_args, mesh_struct,
                                new_flags, raise_flags, zeros_i32)
from .mesh_connectivity import scan as _scan   # under the name it has always had here (the atlas tests take it from here)

NAME = "mesh_remesh"


def _target(what: str, h) -> float:
    h = float(h)
    if not math.isfinite(h) or h <= 0:
        raise ValueError(f"{NAME}.{what}: h must be positive and finite")
    return h


def _thresholds(h: float) -> Tuple[float, float]:
    """(lo^2, hi^2) as the header has them"""
    lo, hi = 4.0 / 5.0 * h, 4.0 / 3.0 * h
    return lo * lo, hi * hi


def _conn(what, v, t, conn: Optional[Connectivity]) -> Connectivity:
    if conn is None:
        return build_connectivity(t, v.shape[0], f"{NAME}.{what}")
    if conn.V != v.shape[0] or conn.F != t.shape[0] or conn.tri.data_ptr() != t.data_ptr():
        raise ValueError(f"{NAME}.{what}: the connectivity does not belong to this mesh")
    return conn


# ---- the single passes ------------------------------------------------------------------------------------------------------

def split_long_edges(vertices, indices, h, conn: Optional[Connectivity] = None):
    """Split every edge longer than 4/3 h at its midpoint: ``(vertices [V+S,3], indices int32, S)``."""
    v, t = mesh_args(f"{NAME}.split_long_edges", vertices, indices)
    h = _target("split_long_edges", h)
    if t.shape[0] == 0:
        return v, t, 0
    c = _conn("split_long_edges", v, t, conn)
    dev = v.device
    mark, count = empty_i32(c.E, dev), empty_i32(c.F, dev)
    launch("gd_mesh_remesh_split_mark", dev, c.V, c.E, v, c.ev, _thresholds(h)[1], mark)
    launch("gd_mesh_remesh_split_count", dev, c.F, c.E, c.fe, mark, count)
    escan, fscan = _scan(mark), _scan(count)
    S, F2 = torch.stack((escan[-1], fscan[-1])).tolist()
    if S == 0:
        return v, t, 0
    flags = new_flags(dev)
    v2 = torch.empty((c.V + S, 3), dtype=torch.float32, device=dev)
    v2[:c.V] = v
    t2 = torch.empty((F2, 3), dtype=torch.int32, device=dev)
    launch("gd_mesh_remesh_split_apply", dev, c.V, c.F, c.E, c.V + S, F2, v, t, c.ev, c.fe, mark, escan, fscan, v2, t2, flags)
    raise_flags(f"{NAME}.split_long_edges", flags.tolist())
    return v2, t2, S


def collapse_short_edges_round(vertices, indices, h, conn: Optional[Connectivity] = None):
    """One round of collapses of edges shorter than 4/5 h: ``(indices int32 with the dead faces removed, collapsed)``.
    Vertices keep their indices (``compact_vertices`` drops the removed ones)."""
    v, t = mesh_args(f"{NAME}.collapse_short_edges_round", vertices, indices)
    h = _target("collapse_short_edges_round", h)
    if t.shape[0] == 0:
        return t, 0
    c = _conn("collapse_short_edges_round", v, t, conn)
    dev = v.device
    lo2, hi2 = _thresholds(h)
    m = mesh_struct(v, c)
    direction = empty_i32(c.E, dev)
    ekey = torch.empty(c.E, dtype=torch.int64, device=dev)
    vkey = torch.full((c.V,), -1, dtype=torch.int64, device=dev)        # all ones: above every key
    remap = torch.arange(c.V, dtype=torch.int32, device=dev)
    flags = new_flags(dev)
    launch("gd_mesh_remesh_collapse_candidates", dev, m, lo2, hi2, direction, ekey, vkey)
    launch("gd_mesh_remesh_collapse_select", dev, m, direction, ekey, vkey, remap, flags)
    return drop_dead_faces(f"{NAME}.collapse_short_edges_round", t, remap, flags)


def flip_edges_round(vertices, indices, conn: Optional[Connectivity] = None):
    """One round of valence-improving edge flips: ``(indices int32, flipped)``."""
    v, t = mesh_args(f"{NAME}.flip_edges_round", vertices, indices)
    if t.shape[0] == 0:
        return t, 0
    c = _conn("flip_edges_round", v, t, conn)
    dev = v.device
    quad = empty_i32(4 * c.E, dev)
    ekey = torch.empty(c.E, dtype=torch.int64, device=dev)
    vkey = torch.full((c.V,), -1, dtype=torch.int64, device=dev)
    flags = new_flags(dev)
    out = t.clone()
    launch("gd_mesh_remesh_flip_candidates", dev, mesh_struct(v, c), quad, ekey, vkey)
    launch("gd_mesh_remesh_flip_apply", dev, c.V, c.F, c.E, c.eh, quad, ekey, vkey, out, flags)
    got = flags.tolist()
    raise_flags(f"{NAME}.flip_edges_round", got)
    n = got[_native.REMESH_FLAG_SELECTED]
    return (out, n) if n else (t, 0)


def tangential_relax(vertices, indices, conn: Optional[Connectivity] = None):
    """One Jacobi step of tangential smoothing: ``(vertices, moved int32 [V])``; boundary and isolated vertices stay."""
    v, t = mesh_args(f"{NAME}.tangential_relax", vertices, indices)
    if t.shape[0] == 0:
        return v, zeros_i32(v.shape[0], v.device)
    c = _conn("tangential_relax", v, t, conn)
    out, moved = torch.empty_like(v), empty_i32(c.V, v.device)
    launch("gd_mesh_remesh_relax", v.device, mesh_struct(v, c), out, moved)
    return out, moved


class SurfaceGrid(NamedTuple):
    """a surface binned for ``project_to_surface``"""
    vertices: torch.Tensor
    indices: torch.Tensor
    grid: object            # _native.RemeshGrid
    cell: float
    start: torch.Tensor     # int32 [cells+1]
    items: torch.Tensor     # int32 [capacity]


def build_surface_grid(vertices, indices, min_cell: float = 0.0) -> SurfaceGrid:
    """Bin the triangles of a surface by bounding box into a uniform grid whose cell is at least its longest edge and
    ``min_cell``, doubled until the grid has at most 2^21 cells (the rule of the header).  Two host reads."""
    what = "build_surface_grid"
    v, t = mesh_args(f"{NAME}.{what}", vertices, indices)
    if t.shape[0] == 0:
        raise ValueError(f"{NAME}.{what}: the surface has no triangle")
    dev, V, F = v.device, v.shape[0], t.shape[0]
    c = build_connectivity(t, V, f"{NAME}.{what}")
    lengths = torch.empty(c.E, dtype=torch.float32, device=dev)
    launch("gd_mesh_remesh_edge_lengths", dev, V, c.E, v, c.ev.to(torch.int64), lengths)
    box = torch.cat((v.amin(0), v.amax(0), lengths.max()[None])).tolist()
    if not all(math.isfinite(x) for x in box):
        raise ValueError(f"{NAME}.{what}: the surface has a position that is not finite")
    cell = max(box[6], float(min_cell), 1e-30)
    cell = float(torch.tensor(cell, dtype=torch.float32)) * (1.0 + 2.0 ** -20)   # never below the longest edge in fp32
    extent = [box[3 + a] - box[a] for a in range(3)]
    while True:
        dims = [int(extent[a] / cell) + 1 for a in range(3)]
        if dims[0] * dims[1] * dims[2] <= _native.REMESH_MAX_CELLS:
            break
        cell *= 2.0
    grid = _native.RemeshGrid((C.c_float * 3)(*box[:3]), cell, (C.c_int32 * 3)(*dims))
    cells = dims[0] * dims[1] * dims[2]
    flags, count = new_flags(dev), zeros_i32(cells, dev)
    capacity = 8 * F                                                    # a box no wider than a cell touches <= 2 per axis
    items = zeros_i32(capacity, dev)
    launch("gd_mesh_remesh_grid_bin", dev, C.byref(grid), V, F, v, t, 0, count, None, None, 0, flags)
    start = _scan(count)
    count.zero_()
    launch("gd_mesh_remesh_grid_bin", dev, C.byref(grid), V, F, v, t, 1, count, start, items, capacity, flags)
    raise_flags(f"{NAME}.{what}", flags.tolist())
    return SurfaceGrid(v, t, grid, cell, start, items)


def project_to_surface(vertices, surface: SurfaceGrid, moved: Optional[torch.Tensor] = None):
    """Each vertex (each with ``moved`` != 0, if given) goes to its closest point on ``surface``; one with no triangle
    within the grid's cell keeps its position: ``(vertices, number of those)``."""
    what = "project_to_surface"
    v = require_gpu(f"{NAME}.{what}", "vertices", vertices, torch.float32, 3).detach().contiguous()
    if not isinstance(surface, SurfaceGrid):
        raise TypeError(f"{NAME}.{what}: surface must be the SurfaceGrid of build_surface_grid")
    if moved is not None:
        moved = require_gpu(f"{NAME}.{what}", "moved", moved, torch.int32)
        if moved.shape != (v.shape[0],):
            raise ValueError(f"{NAME}.{what}: moved must be [V]")
    if v.shape[0] == 0:
        return v, 0
    dev = v.device
    out, flags = torch.empty_like(v), new_flags(dev)
    launch("gd_mesh_remesh_project", dev, C.byref(surface.grid), v.shape[0], v, moved, surface.vertices.shape[0],
           surface.indices.shape[0], surface.vertices, surface.indices, surface.start, surface.items,
           surface.items.shape[0], out, flags)
    return out, flags.tolist()[_native.REMESH_FLAG_UNPROJECTED]


def compact_vertices(vertices, indices):
    """Drop the vertices no face names, preserving order: ``(vertices, indices int32)``."""
    v, t = mesh_args(f"{NAME}.compact_vertices", vertices, indices)
    dev, V, F = v.device, v.shape[0], t.shape[0]
    if F == 0:
        return v[:0], t
    flags, used = new_flags(dev), zeros_i32(V, dev)
    launch("gd_mesh_remesh_used_vertices", dev, V, F, t, used, flags)
    used_scan = _scan(used)
    got = torch.cat((used_scan[-1:], flags)).tolist()
    raise_flags(f"{NAME}.compact_vertices", got[1:])
    if got[0] == V:
        return v, t
    v2, t2 = torch.empty((got[0], 3), dtype=torch.float32, device=dev), torch.empty_like(t)
    launch("gd_mesh_remesh_compact_vertices", dev, V, F, got[0], v, t, used, used_scan, v2, t2, flags)
    raise_flags(f"{NAME}.compact_vertices", flags.tolist())
    return v2, t2


def mean_edge_length(vertices, geo) -> torch.Tensor:
    """The mean length of ``geo.edges`` (a ``mesh_geometry.MeshGeometry``) at ``vertices``: a float32 scalar on the device."""
    v = require_gpu(f"{NAME}.mean_edge_length", "vertices", vertices, torch.float32, 3).detach().contiguous()
    edges = require_gpu(f"{NAME}.mean_edge_length", "geo.edges", geo.edges, torch.int64, 2).contiguous()
    if edges.shape[0] == 0:
        raise ValueError(f"{NAME}.mean_edge_length: the mesh has no edge")
    lengths = torch.empty(edges.shape[0], dtype=torch.float32, device=v.device)
    launch("gd_mesh_remesh_edge_lengths", v.device, v.shape[0], edges.shape[0], v, edges, lengths)
    return lengths.mean()


# ---- the whole remesh -------------------------------------------------------------------------------------------------------

def remesh_botsch(vertices, indices, h, iterations: int = 10, project: bool = True, rounds: int = 4):
    """Isotropic remeshing towards edge length ``h``: ``(vertices float32 [V',3], indices int32 [F',3], info)``.
    ``info[kind]`` for kind in split / collapsed / flipped / unprojected is a list with one Python int per iteration.
    ``ValueError`` for a bad ``h``, an index out of range, a non-manifold mesh or a face that lists a vertex twice.
    Vertices no face names are dropped."""
    what = "remesh_botsch"
    v, t = mesh_args(f"{NAME}.{what}", vertices, indices)
    h = _target(what, h)
    iterations, rounds = int(iterations), int(rounds)
    if iterations < 0 or rounds < 0:
        raise ValueError(f"{NAME}.{what}: iterations and rounds must be >= 0")
    info: Dict[str, List[int]] = {"split": [], "collapsed": [], "flipped": [], "unprojected": []}
    if t.shape[0] == 0:
        return v[:0].clone(), t.clone(), info
    conn = build_connectivity(t, v.shape[0], f"{NAME}.{what}")          # the input's own errors, before anything moves
    v, t2 = compact_vertices(v, t)
    conn = conn if t2.data_ptr() == t.data_ptr() else None
    t = t2
    surface = build_surface_grid(v, t, min_cell=4.0 / 3.0 * h) if project and iterations else None
    for _ in range(iterations):
        v, t2, n = split_long_edges(v, t, h, conn)
        conn = conn if t2.data_ptr() == t.data_ptr() else None
        t = t2
        info["split"].append(n)
        total = 0
        for _ in range(rounds):
            t2, n = collapse_short_edges_round(v, t, h, conn)
            conn = conn if t2.data_ptr() == t.data_ptr() else None
            t = t2
            total += n
            if n == 0:
                break
        info["collapsed"].append(total)
        if total:
            v, t = compact_vertices(v, t)
            conn = None
        total = 0
        for _ in range(rounds):
            conn = _conn(what, v, t, conn)
            t2, n = flip_edges_round(v, t, conn)
            conn = conn if t2.data_ptr() == t.data_ptr() else None
            t = t2
            total += n
            if n == 0:
                break
        info["flipped"].append(total)
        if t.shape[0] == 0:
            info["unprojected"].append(0)
            continue
        conn = _conn(what, v, t, conn)
        v, moved = tangential_relax(v, t, conn)
        n = 0
        if surface is not None:
            v, n = project_to_surface(v, surface, moved)
        info["unprojected"].append(n)
    return v, t, info
