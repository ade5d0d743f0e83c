"""Mesh cleaning on the GPU: the place of kiui's ``clean_mesh`` (a chain of MeshLab filters: remove unreferenced vertices,
merge close vertices, remove duplicate and null faces, remove small components by diameter and by face count, repair
non-manifold edges by removing faces and non-manifold vertices by splitting), which the reference's NeTF stage calls on the
mesh it loads (``Garment_Deformer_NeTF/netf/render/mesh_renderer.py:114-121`` and ``:330``), on the HIP kernels of
``csrc/raster_clean.hip`` (C-ABI and definitions: include/gd_mesh_clean.h) -- no CPU path.

  * ``clean_mesh(vertices, indices, merge_pct=1.0, min_faces=64, min_diameter_pct=20.0, repair=True)``   the whole chain:
        ``CleanResult(vertices, indices, vertex_map, face_map, report)``
  * ``merge_close_vertices(vertices, indices, merge_pct)``                  ``(target int32 [V], rounds)``
  * ``remove_null_faces(vertices, indices)``                                ``(indices', face_map)``
  * ``remove_duplicate_faces(vertices, indices)``                           ``(indices', face_map)``
  * ``face_components(vertices, indices)``                                  ``label int32 [F]``
  * ``remove_small_components(vertices, indices, min_faces, min_diameter_pct)``   ``(indices', face_map)``
  * ``repair_non_manifold_edges(vertices, indices)``                        ``(indices', face_map, rounds)``
  * ``split_non_manifold_vertices(vertices, indices)``                      ``(vertices', indices', copies)``

The single passes are for callers with a schedule of their own; in them a face that names a vertex twice has no edges (it
is a component of its own and never a duplicate), and the percentages refer to the box of the mesh they are given.  The
definitions are the project's own; agreement with MeshLab is unverified.

What is torch here is plumbing: allocation and fills, two ``torch.sort`` calls (the half-edge keys, stable; the keys of the
vertex copies, only when a vertex is split) and the read-backs.  Host reads of a ``clean_mesh``: one for the box, the
counters and the argument flags; one per 16 merge rounds; one per 2 component sweeps; with ``repair`` one per 4 edge rounds
and one per 2 fan sweeps; one for the sizes of the output.  That is 6 at the least (one batch of each); 8 on the 200 000-face
mesh of tools/clean_time.py, whose labels and fans take a second batch of sweeps each."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _native
from ._launch import launch
from .mesh_connectivity import empty_i32, mesh_args, scan, zeros_i32

NAME = "mesh_clean"
MERGE_ROUNDS = _native.CLEAN_MAX_ROUNDS   # rounds between two reads of the undecided count
EDGE_ROUNDS = 4
SWEEPS = 2
REPORT_KEYS = ("unreferenced", "merged", "merge_rounds", "null_faces", "duplicate_faces", "components", "components_removed",
               "component_faces_removed", "edge_faces_removed", "edge_rounds", "vertices_split")


class CleanResult(NamedTuple):
    vertices: torch.Tensor      # float32 [V',3]
    indices: torch.Tensor       # int32 [F',3]
    vertex_map: torch.Tensor    # int32 [V]: the output row of each input vertex, -1 if nothing names it any more
    face_map: torch.Tensor      # int32 [F']: the input face of each output face
    report: Dict[str, int]


class EdgeTable(NamedTuple):
    """the sorted half-edge keys of include/gd_mesh_clean.h section 4"""
    skeys: torch.Tensor         # int64 [3F]
    she: torch.Tensor           # int32 [3F]
    pos: torch.Tensor           # int32 [3F]


def _args(what: str, vertices, indices) -> Tuple[torch.Tensor, torch.Tensor]:
    """``mesh_connectivity.mesh_args``; a tensor that is not on the GPU is a ``ValueError`` here"""
    for t in (vertices, indices):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{NAME}.{what}: the HIP kernels have no CPU path (vertices and indices must be on the GPU)")
    return mesh_args(f"{NAME}.{what}", vertices, indices)


def _stats(dev) -> torch.Tensor:
    return torch.zeros(_native.CLEAN_STATS, dtype=torch.int32, device=dev)


def _check(what: str, v: torch.Tensor, t: torch.Tensor, stats: torch.Tensor):
    """``(used int32 [V], box as six floats, diagonal float64, referenced)``; the argument errors of section 0.  One host
    read."""
    dev, V, F = v.device, v.shape[0], t.shape[0]
    used, box = empty_i32(V, dev), torch.empty(6, dtype=torch.float32, device=dev)
    launch("gd_mesh_clean_check", dev, V, F, v, t, used, box, empty_i32(6, dev), stats)
    got = torch.cat((box.view(torch.int32), stats)).cpu().numpy()
    flags = got[6:]
    if flags[_native.CLEAN_STAT_INDEX]:
        raise ValueError(f"{NAME}.{what}: vertex index out of range")
    if flags[_native.CLEAN_STAT_NONFINITE]:
        raise ValueError(f"{NAME}.{what}: a position is not finite on a vertex some face references")
    box = [float(x) for x in got[:6].view(np.float32)]
    d = [box[3 + a] - box[a] for a in range(3)]
    diagonal = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return used, box, diagonal, int(flags[_native.CLEAN_STAT_REFERENCED])


def _fraction(what: str, diagonal: float, pct: float) -> np.float32:
    """(float) (D pct / 100)"""
    with np.errstate(over="ignore"):
        x = np.float32(diagonal * float(pct) / 100.0)
        if not np.isfinite(x) or not np.isfinite(x * x):
            raise ValueError(f"{NAME}.{what}: the bounding box is too large for a percentage of its diagonal in float32")
    return x


def _grid(box, r: float):
    """the grid of section 2 for the radius ``r``: ``(gd_remesh_grid, cells)``"""
    cell = float(np.float32(max(float(r), 2.0 ** -60))) * (1.0 + 2.0 ** -20)
    extent = [box[3 + a] - box[a] for a in range(3)]
    while True:
        dims = [int(extent[a] / cell) + 1 for a in range(3)]
        if dims[0] * dims[1] * dims[2] <= _native.CLEAN_MAX_CELLS:
            break
        cell *= 2.0
    return _native.RemeshGrid((C.c_float * 3)(*box[:3]), cell, (C.c_int32 * 3)(*dims)), dims[0] * dims[1] * dims[2]


def _merge(what: str, v, used, box, diagonal: float, merge_pct: float, stats) -> Tuple[torch.Tensor, int]:
    """``(target int32 [V], rounds)`` of section 2; one host read per ``MERGE_ROUNDS`` rounds"""
    dev, V = v.device, v.shape[0]
    target = empty_i32(V, dev)
    if not merge_pct > 0:
        launch("gd_mesh_clean_merge_target", dev, None, V, v, used, None, None, 0.0, 0, None, target, stats)
        return target, 0
    r = _fraction(what, diagonal, merge_pct)
    r2 = float(r * r)
    grid, cells = _grid(box, float(r))
    g = C.byref(grid)
    count, items = zeros_i32(cells, dev), empty_i32(V, dev)
    launch("gd_mesh_clean_grid_bin", dev, g, V, v, used, 0, count, None, None)
    start = scan(count)
    count.zero_()
    launch("gd_mesh_clean_grid_bin", dev, g, V, v, used, 1, count, start, items)
    state, other, undecided = zeros_i32(V, dev), empty_i32(V, dev), empty_i32(MERGE_ROUNDS, dev)
    rounds = 0
    while True:                                                         # V rounds always suffice: no cap
        launch("gd_mesh_clean_merge_rounds", dev, g, V, v, used, start, items, r2, MERGE_ROUNDS, state, other, undecided)
        left = undecided.tolist()
        if 0 in left:
            rounds += left.index(0) + 1
            break
        rounds += MERGE_ROUNDS
    launch("gd_mesh_clean_merge_target", dev, g, V, v, used, start, items, r2, 1, state, target, stats)
    return target, rounds


def _relabel(v, t, target: Optional[torch.Tensor], stats):
    """``(tri int32 [F,3], alive int32 [F], akey float32 [F])`` of section 3"""
    dev, F = v.device, t.shape[0]
    tri, alive, akey = torch.empty_like(t), empty_i32(F, dev), torch.empty(F, dtype=torch.float32, device=dev)
    launch("gd_mesh_clean_relabel", dev, v.shape[0], F, v, t, target, tri, alive, akey, stats)
    return tri, alive, akey


def _edge_table(tri: torch.Tensor, alive: torch.Tensor, V: int) -> EdgeTable:
    dev, F = tri.device, tri.shape[0]
    hkeys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    launch("gd_mesh_clean_edge_keys", dev, V, F, tri, alive, hkeys)
    skeys, order = torch.sort(hkeys, stable=True)
    she, pos = empty_i32(3 * F, dev), empty_i32(3 * F, dev)
    launch("gd_mesh_clean_edge_table", dev, 3 * F, skeys, order, she, pos)
    return EdgeTable(skeys, she, pos)


def _duplicates(tri, alive, table: EdgeTable, stats) -> torch.Tensor:
    out = torch.empty_like(alive)
    launch("gd_mesh_clean_duplicates", tri.device, tri.shape[0], tri, alive, table.skeys, table.she, table.pos, out, stats)
    return out


def _sweeps(what: str, entry: str, dev, n: int, args, count: Optional[list] = None) -> torch.Tensor:
    """hooking with pointer jumping until a sweep changes nothing: ``parent int32 [n]``; one host read per ``SWEEPS``
    sweeps.  ``count``, a list, receives the number of sweeps up to and including the first that changed nothing."""
    parent, changed = empty_i32(n, dev), empty_i32(SWEEPS, dev)
    for done in range(0, _native.ATLAS_MAX_SWEEPS, SWEEPS):
        launch(entry, dev, *args, SWEEPS, 1 if done == 0 else 0, parent, changed)
        got = changed.tolist()
        if not got[-1]:
            if count is not None:
                count.append(done + got.index(0) + 1)
            return parent
    raise RuntimeError(f"{NAME}.{what}: the components still changed after {_native.ATLAS_MAX_SWEEPS} sweeps")


def _face_parents(what: str, tri, alive, table: EdgeTable, count: Optional[list] = None) -> torch.Tensor:
    F = tri.shape[0]
    return _sweeps(what, "gd_mesh_clean_face_sweeps", tri.device, F, (F, table.skeys, table.she, alive), count)


def _component_filter(v, tri, alive, parent, min_faces: int, t2: float, stats):
    """``(label int32 [F], alive' int32 [F])`` of section 5"""
    dev, F = tri.device, tri.shape[0]
    ckeys, ccount = torch.empty(6 * F, dtype=torch.int32, device=dev), empty_i32(F, dev)
    launch("gd_mesh_clean_component_stats", dev, v.shape[0], F, v, tri, alive, parent, ckeys, ccount)
    label, out = empty_i32(F, dev), empty_i32(F, dev)
    launch("gd_mesh_clean_component_filter", dev, F, alive, parent, ckeys, ccount, int(min_faces), float(t2), label, out, stats)
    return label, out


def _edge_rounds(alive, akey, table: EdgeTable) -> Tuple[torch.Tensor, int]:
    """``(alive' int32 [F], rounds)`` of section 6; one host read per ``EDGE_ROUNDS`` rounds"""
    dev, F = alive.device, alive.shape[0]
    live, other, over = alive.clone(), empty_i32(F, dev), empty_i32(EDGE_ROUNDS, dev)
    rounds = 0
    while True:                                                         # every round with work to do removes a face: no cap
        launch("gd_mesh_clean_edge_rounds", dev, F, table.skeys, table.she, akey, EDGE_ROUNDS, live, other, over)
        found = over.tolist()
        if 0 in found:
            return live, rounds + found.index(0)
        rounds += EDGE_ROUNDS


def _corner_parents(what: str, tri, alive, table: EdgeTable) -> torch.Tensor:
    F = tri.shape[0]
    return _sweeps(what, "gd_mesh_clean_corner_sweeps", tri.device, 3 * F, (F, tri, table.skeys, table.she, alive))


def _emit(v, tri, alive, target: Optional[torch.Tensor], cparent: Optional[torch.Tensor], stats):
    """Section 8: ``(vertices, indices, vertex_map, face_map, stats as a list)``.  One host read."""
    dev, V, F = v.device, v.shape[0], tri.shape[0]
    used = empty_i32(V, dev)
    vmin = split_key = None
    if cparent is not None:
        vmin, split_key = empty_i32(V, dev), torch.empty(3 * F, dtype=torch.int64, device=dev)
    launch("gd_mesh_clean_fan_roots", dev, V, F, tri, alive, cparent, vmin, used, split_key, stats)
    fscan, vscan = scan(alive), scan(used)
    got = torch.cat((fscan[-1:], vscan[-1:], stats)).tolist()
    Fout, V0, S = got[0], got[1], got[2 + _native.CLEAN_STAT_SPLIT]
    if Fout == 0:
        return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev),
                torch.full((V,), -1, dtype=torch.int32, device=dev), empty_i32(0, dev), got[2:])
    crank = sorted_keys = None
    if S > 0:
        sorted_keys = torch.sort(split_key).values
        crank = empty_i32(3 * F, dev)
        launch("gd_mesh_clean_fan_ranks", dev, 3 * F, S, sorted_keys, crank)
    verts_out = torch.empty((V0 + S, 3), dtype=torch.float32, device=dev)
    tri_out = torch.empty((Fout, 3), dtype=torch.int32, device=dev)
    face_map, vertex_map = empty_i32(Fout, dev), empty_i32(V, dev)
    launch("gd_mesh_clean_emit", dev, V, F, Fout, V0, S, v, tri, alive, fscan, used, vscan, target,
           cparent if S > 0 else None, crank, sorted_keys, verts_out, tri_out, face_map, vertex_map)
    return verts_out, tri_out, vertex_map, face_map, got[2:]


def _compact_faces(t: torch.Tensor, alive: torch.Tensor):
    """``(t[alive != 0], face_map)``, the vertices untouched.  One host read."""
    dev, F = t.device, t.shape[0]
    fscan = scan(alive)
    Fout = int(fscan[-1])
    face_map, out = empty_i32(Fout, dev), torch.empty((Fout, 3), dtype=torch.int32, device=dev)
    if Fout:
        launch("gd_mesh_clean_compact_faces", dev, F, Fout, t, alive, fscan, out, face_map)
    return out, face_map


def _empty_report(V: int) -> Dict[str, int]:
    report = {k: 0 for k in REPORT_KEYS}
    report["unreferenced"] = V
    return report


# ---- the whole chain ----------------------------------------------------------------------------------------------------------

def clean_mesh(vertices, indices, merge_pct: float = 1.0, min_faces: int = 64, min_diameter_pct: float = 20.0,
               repair: bool = True) -> CleanResult:
    """Clean a triangle mesh by the steps of include/gd_mesh_clean.h in their order: drop unreferenced vertices, weld the
    vertices within ``merge_pct`` percent of the bounding-box diagonal, drop null and duplicate faces, drop the connected
    components with fewer than ``min_faces`` faces or a box diagonal below ``min_diameter_pct`` percent, and with ``repair``
    remove faces until no edge has more than two and give every fan of a pinched vertex a vertex of its own.  A criterion
    that is ``<= 0`` is off.  The diagonal is measured once, on the input.  Every output position is bitwise an input
    position; face orientation is not repaired.  ``F == 0`` returns the empty mesh.  ``ValueError`` for a tensor that is
    not on the GPU, an index out of range, a position that is not finite on a referenced vertex or a percentage that is not
    finite; nothing has been written by then."""
    what = "clean_mesh"
    v, t = _args(what, vertices, indices)
    merge_pct, min_faces, min_diameter_pct = float(merge_pct), int(min_faces), float(min_diameter_pct)
    if not math.isfinite(merge_pct) or not math.isfinite(min_diameter_pct):
        raise ValueError(f"{NAME}.{what}: merge_pct and min_diameter_pct must be finite")
    dev, V, F = v.device, v.shape[0], t.shape[0]
    if F == 0:
        return CleanResult(v[:0].clone(), t.clone(), torch.full((V,), -1, dtype=torch.int32, device=dev), empty_i32(0, dev),
                           _empty_report(V))
    stats = _stats(dev)
    used, box, diagonal, referenced = _check(what, v, t, stats)
    threshold = _fraction(what, diagonal, min_diameter_pct) if min_diameter_pct > 0 else np.float32(0)
    target, merge_rounds = _merge(what, v, used, box, diagonal, merge_pct, stats)
    tri, alive, akey = _relabel(v, t, target, stats)
    table = _edge_table(tri, alive, V)
    alive = _duplicates(tri, alive, table, stats)
    parent = _face_parents(what, tri, alive, table)
    _, alive = _component_filter(v, tri, alive, parent, min_faces, float(threshold * threshold), stats)
    edge_rounds, cparent = 0, None
    if repair:
        alive, edge_rounds = _edge_rounds(alive, akey, table)
        cparent = _corner_parents(what, tri, alive, table)
    v2, t2, vertex_map, face_map, got = _emit(v, tri, alive, target, cparent, stats)
    removed = got[_native.CLEAN_STAT_NULL] + got[_native.CLEAN_STAT_DUPLICATE] + got[_native.CLEAN_STAT_COMPONENT_FACES]
    report = {"unreferenced": V - referenced, "merged": got[_native.CLEAN_STAT_MERGED], "merge_rounds": merge_rounds,
              "null_faces": got[_native.CLEAN_STAT_NULL], "duplicate_faces": got[_native.CLEAN_STAT_DUPLICATE],
              "components": got[_native.CLEAN_STAT_COMPONENTS],
              "components_removed": got[_native.CLEAN_STAT_COMPONENTS_REMOVED],
              "component_faces_removed": got[_native.CLEAN_STAT_COMPONENT_FACES],
              "edge_faces_removed": F - removed - int(t2.shape[0]), "edge_rounds": edge_rounds,
              "vertices_split": got[_native.CLEAN_STAT_SPLIT]}
    return CleanResult(v2, t2, vertex_map, face_map, {k: int(report[k]) for k in REPORT_KEYS})


# ---- the single passes --------------------------------------------------------------------------------------------------------

def _start(what: str, vertices, indices):
    """the arguments, checked: ``(v, t, stats, used, box, diagonal)``; ``None`` in place of the last four when F == 0"""
    v, t = _args(what, vertices, indices)
    if t.shape[0] == 0:
        return v, t, None, None, None, None
    stats = _stats(v.device)
    used, box, diagonal, _ = _check(what, v, t, stats)
    return v, t, stats, used, box, diagonal


def _whole(t: torch.Tensor) -> torch.Tensor:
    return torch.ones(t.shape[0], dtype=torch.int32, device=t.device)


def merge_close_vertices(vertices, indices, merge_pct: float = 1.0) -> Tuple[torch.Tensor, int]:
    """Section 2 alone: ``(target int32 [V], rounds)``; ``target[v]`` is the vertex v is welded to (v itself for a centre),
    -1 for a vertex no face names."""
    what = "merge_close_vertices"
    v, t, stats, used, box, diagonal = _start(what, vertices, indices)
    if not math.isfinite(float(merge_pct)):
        raise ValueError(f"{NAME}.{what}: merge_pct must be finite")
    if stats is None:
        return torch.full((v.shape[0],), -1, dtype=torch.int32, device=v.device), 0
    return _merge(what, v, used, box, diagonal, float(merge_pct), stats)


def remove_null_faces(vertices, indices) -> Tuple[torch.Tensor, torch.Tensor]:
    """Section 3 alone: ``(indices int32 [F',3], face_map int32 [F'])``"""
    v, t, stats, *_ = _start("remove_null_faces", vertices, indices)
    if stats is None:
        return t.clone(), empty_i32(0, v.device)
    _, alive, _ = _relabel(v, t, None, stats)
    return _compact_faces(t, alive)


def remove_duplicate_faces(vertices, indices) -> Tuple[torch.Tensor, torch.Tensor]:
    """Section 4 alone: of the faces with one unordered vertex triple the lowest index stays"""
    v, t, stats, *_ = _start("remove_duplicate_faces", vertices, indices)
    if stats is None:
        return t.clone(), empty_i32(0, v.device)
    alive = _whole(t)
    return _compact_faces(t, _duplicates(t, alive, _edge_table(t, alive, v.shape[0]), stats))


def face_components(vertices, indices, return_sweeps: bool = False):
    """``label int32 [F]``: the lowest face index of the edge-connected component of each face; with ``return_sweeps``
    ``(label, sweeps)``, the hooking sweeps it took, the last of which changed nothing (not reproducible: it follows the
    schedule of the hooks)."""
    what = "face_components"
    v, t, stats, *_ = _start(what, vertices, indices)
    if stats is None:
        return (empty_i32(0, v.device), 0) if return_sweeps else empty_i32(0, v.device)
    alive, count = _whole(t), []
    parent = _face_parents(what, t, alive, _edge_table(t, alive, v.shape[0]), count)
    label = _component_filter(v, t, alive, parent, 0, 0.0, stats)[0]
    return (label, count[0]) if return_sweeps else label


def remove_small_components(vertices, indices, min_faces: int = 64, min_diameter_pct: float = 20.0):
    """Section 5 alone: ``(indices', face_map)`` without the components below either threshold"""
    what = "remove_small_components"
    v, t, stats, _, _, diagonal = _start(what, vertices, indices)
    if not math.isfinite(float(min_diameter_pct)):
        raise ValueError(f"{NAME}.{what}: min_diameter_pct must be finite")
    if stats is None:
        return t.clone(), empty_i32(0, v.device)
    threshold = _fraction(what, diagonal, min_diameter_pct) if float(min_diameter_pct) > 0 else np.float32(0)
    alive = _whole(t)
    parent = _face_parents(what, t, alive, _edge_table(t, alive, v.shape[0]))
    return _compact_faces(t, _component_filter(v, t, alive, parent, int(min_faces), float(threshold * threshold), stats)[1])


def repair_non_manifold_edges(vertices, indices):
    """Section 6 alone: ``(indices', face_map, rounds)``; no edge of the result has more than two faces"""
    v, t, stats, *_ = _start("repair_non_manifold_edges", vertices, indices)
    if stats is None:
        return t.clone(), empty_i32(0, v.device), 0
    alive = _whole(t)
    akey = _relabel(v, t, None, stats)[2]
    alive, rounds = _edge_rounds(alive, akey, _edge_table(t, alive, v.shape[0]))
    return _compact_faces(t, alive) + (rounds,)


def split_non_manifold_vertices(vertices, indices):
    """Section 7 alone: ``(vertices', indices', copies)``; every vertex of the result has one fan.  Vertices no face names
    are dropped."""
    what = "split_non_manifold_vertices"
    v, t, stats, *_ = _start(what, vertices, indices)
    if stats is None:
        return v[:0].clone(), t.clone(), 0
    alive = _whole(t)
    cparent = _corner_parents(what, t, alive, _edge_table(t, alive, v.shape[0]))
    v2, t2, _, _, got = _emit(v, t, alive, None, cparent, stats)
    return v2, t2, int(got[_native.CLEAN_STAT_SPLIT])
