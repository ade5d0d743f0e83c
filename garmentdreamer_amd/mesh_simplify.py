"""The deformer's final mesh on the GPU: the place of ``write_mesh(..., post_process=True)`` in the reference
(``Garment_Deformer_NeTF/deformer/utils/io.py:18-36``, ``deformer/tools/post_process.py:13-38``: rotate, MeshLab's quadric
edge-collapse decimation to 40 000 faces with the boundary preserved and endpoint placement, Taubin smoothing), on the HIP
kernels of ``csrc/raster_simplify.hip`` (C-ABI and definitions: include/gd_mesh_simplify.h) -- no CPU path.

  * ``decimate_quadric(vertices, indices, target_faces, passes=4, max_rounds=1024)``   quadric-error half-edge collapses in
        rounds of independent sets; the boundary comes back exactly
  * ``taubin_smooth(vertices, indices, steps=10, lam=0.5, mu=-0.53)``                  ``steps`` x (a lam pass, a mu pass)
  * ``rotate_upright(vertices)``                                                       (x, y, z) -> (x, z, -y), exactly
  * ``post_process_mesh(vertices, indices, target_faces=40000, smooth=True, rotate=True)``   the three in the reference's order
  * ``write_obj(path, vertices, indices)``                                             plain ``v`` / ``f`` lines

What is torch here is plumbing: allocation and fills, one ``torch.sort`` of the candidate keys per round, and the read-back
of counts.  The connectivity, the relabelling and the compaction are those of ``mesh_connectivity``, unchanged.  Host reads
per round: three (the connectivity build's edge count and flags; the faces left and the selected count; the compaction's
flags).  Agreement with MeshLab is unverified."""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import torch

from ._launch import launch
from .mesh_connectivity import (Connectivity, build_connectivity, drop_dead_faces, mesh_args, mesh_struct, new_flags,
                                zeros_i32)
from .mesh_remesh import compact_vertices

NAME = "mesh_simplify"


def _mesh_args(what: str, vertices, indices) -> Tuple[torch.Tensor, torch.Tensor]:
    """``mesh_connectivity.mesh_args``; a tensor that is not on the GPU is a ``ValueError`` here"""
    for t in (vertices, indices):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{NAME}.{what}: the HIP kernels have no CPU path (vertices and indices must be on the GPU)")
    return mesh_args(f"{NAME}.{what}", vertices, indices)


def vertex_quadrics(vertices: torch.Tensor, conn: Connectivity) -> torch.Tensor:
    """float64 [V,10]: the sum of the face quadrics of each vertex, in the order of its ``vf`` row"""
    q = torch.empty((conn.V, 10), dtype=torch.float64, device=vertices.device)
    launch("gd_mesh_simplify_quadrics", vertices.device, mesh_struct(vertices, conn), q)
    return q


def collapse_candidates(vertices: torch.Tensor, conn: Connectivity, quadrics: torch.Tensor):
    """``(key int64 [E], direction int32 [E], cost float64 [E,2])`` of the header's candidate pass"""
    dev = vertices.device
    key = torch.empty(conn.E, dtype=torch.int64, device=dev)
    direction = torch.empty(conn.E, dtype=torch.int32, device=dev)
    cost = torch.empty((conn.E, 2), dtype=torch.float64, device=dev)
    launch("gd_mesh_simplify_candidates", dev, mesh_struct(vertices, conn), quadrics, key, direction, cost)
    return key, direction, cost


def decimation_round(vertices: torch.Tensor, indices: torch.Tensor, quadrics: torch.Tensor, target_faces: int, passes: int = 4,
                     conn: Connectivity = None):
    """One round towards ``target_faces`` on one connectivity: ``(indices int32 with the dead faces removed, selected)``.
    ``vertices`` float32 [V,3] and ``indices`` int32 [F,3] contiguous on the GPU, F > ``target_faces``; ``quadrics`` is
    updated in place; vertices keep their indices."""
    what = "decimation_round"
    dev, V, F = vertices.device, vertices.shape[0], indices.shape[0]
    c = conn if conn is not None else build_connectivity(indices, V, f"{NAME}.{what}")
    m = mesh_struct(vertices, c)
    key, direction, _ = collapse_candidates(vertices, c, quadrics)
    budget = (F - int(target_faces) + 1) // 2
    threshold = torch.sort(key).values[min(budget, c.E) - 1:]          # a device pointer: no host read
    lock = zeros_i32(V, dev)
    remap = torch.arange(V, dtype=torch.int32, device=dev)
    vkey = torch.empty(V, dtype=torch.int64, device=dev)
    flags = new_flags(dev)
    for _ in range(passes):
        vkey.fill_(-1)                                                  # all ones: above every key
        launch("gd_mesh_simplify_spread", dev, m, key, threshold, lock, vkey)
        launch("gd_mesh_simplify_select", dev, m, key, threshold, direction, vkey, remap, quadrics, lock, flags)
    return drop_dead_faces(f"{NAME}.{what}", indices, remap, flags)


def decimate_quadric(vertices, indices, target_faces: int, passes: int = 4, max_rounds: int = 1024):
    """Decimate to ``target_faces`` faces: ``(vertices float32 [V',3], indices int32 [F',3], info)``.  Every output vertex
    is an input vertex where it was; boundary vertices, positions and edges are kept.  ``info``: ``reached`` (``F' <=
    target_faces``; then ``F' >= target_faces - 1``), and per round ``selected`` (collapses) and ``faces`` (left).  A run
    also ends, with ``reached`` False, at a round that selects nothing or after ``max_rounds``.  A mesh that has no more
    than ``target_faces`` faces comes back unchanged, as copies; otherwise vertices no face names are dropped.
    ``ValueError`` for a tensor that is not on the GPU, an index out of range, a face that lists a vertex twice, a
    non-manifold edge, ``target_faces < 0``, ``passes < 1`` or ``max_rounds < 0``; nothing has been written by then."""
    what = "decimate_quadric"
    v, t = _mesh_args(what, vertices, indices)
    target_faces, passes, max_rounds = int(target_faces), int(passes), int(max_rounds)
    if target_faces < 0:
        raise ValueError(f"{NAME}.{what}: target_faces must be >= 0")
    if passes < 1:
        raise ValueError(f"{NAME}.{what}: passes must be >= 1")
    if max_rounds < 0:
        raise ValueError(f"{NAME}.{what}: max_rounds must be >= 0")
    info: Dict[str, object] = {"reached": True, "selected": [], "faces": []}
    if t.shape[0] == 0:
        return v.clone(), t.clone(), info
    conn = build_connectivity(t, v.shape[0], f"{NAME}.{what}")          # the input's own errors, before anything is written
    if t.shape[0] <= target_faces:
        return v.clone(), t.clone(), info
    quadrics = vertex_quadrics(v, conn)
    while t.shape[0] > target_faces:
        if len(info["selected"]) >= max_rounds:
            info["reached"] = False
            break
        t, n = decimation_round(v, t, quadrics, target_faces, passes, conn)
        conn = None
        info["selected"].append(n)
        info["faces"].append(int(t.shape[0]))
        if n == 0:
            info["reached"] = False
            break
    v2, t2 = compact_vertices(v, t)
    # never the caller's own storage: a run that selected nothing on a mesh without unreferenced vertices changes nothing
    v2 = v2.clone() if v2.data_ptr() == vertices.data_ptr() else v2
    t2 = t2.clone() if t2.data_ptr() == indices.data_ptr() else t2
    return v2, t2, info


def taubin_smooth(vertices, indices, steps: int = 10, lam: float = 0.5, mu: float = -0.53) -> torch.Tensor:
    """Taubin smoothing, ``steps`` x (a ``lam`` pass, a ``mu`` pass) of ``p + w (mean of the neighbours - p)``: float32
    [V,3].  A boundary vertex averages along the boundary only; one without neighbours stays.  The defaults are those
    MeshLab documents for ``apply_coord_taubin_smoothing``.  One launch per pass on one connectivity."""
    what = "taubin_smooth"
    v, t = _mesh_args(what, vertices, indices)
    steps, lam, mu = int(steps), float(lam), float(mu)
    if steps < 0 or not math.isfinite(lam) or not math.isfinite(mu):
        raise ValueError(f"{NAME}.{what}: steps must be >= 0, lam and mu finite")
    if t.shape[0] == 0 or steps == 0:
        return v.clone()
    conn = build_connectivity(t, v.shape[0], f"{NAME}.{what}")
    a, b = v, torch.empty_like(v)
    for _ in range(steps):
        for w in (lam, mu):
            launch("gd_mesh_simplify_smooth", v.device, mesh_struct(a, conn), w, b)
            a, b = b, (torch.empty_like(v) if a is v else a)
    return a


def rotate_upright(vertices) -> torch.Tensor:
    """The reference's rotation by -90 degrees about x as the exact map (x, y, z) -> (x, z, -y)"""
    if not isinstance(vertices, torch.Tensor) or not vertices.is_cuda:
        raise ValueError(f"{NAME}.rotate_upright: the HIP kernels have no CPU path (vertices must be on the GPU)")
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{NAME}.rotate_upright: vertices must be float32 [V,3]")
    v = vertices.detach().contiguous()
    out = torch.empty_like(v)
    if v.shape[0]:
        launch("gd_mesh_simplify_rotate", v.device, v.shape[0], v, out)
    return out


def post_process_mesh(vertices, indices, target_faces: int = 40000, smooth: bool = True, rotate: bool = True):
    """The reference's post-process in its order: rotate upright, decimate to ``target_faces``, Taubin-smooth:
    ``(vertices float32, indices int32, info of decimate_quadric)``."""
    v, t = _mesh_args("post_process_mesh", vertices, indices)
    if t.shape[0]:
        build_connectivity(t, v.shape[0], f"{NAME}.post_process_mesh")    # the input's own errors, before anything is written
    if rotate:
        v = rotate_upright(v)
    v, t, info = decimate_quadric(v, t, target_faces)
    if smooth:
        v = taubin_smooth(v, t)
    return v, t, info


def write_obj(path, vertices, indices) -> None:
    """Write ``v`` and ``f`` lines.  A coordinate is the shortest decimal that reads back as the same double, which is the
    float32 itself: ``template.load_obj`` returns the same float32 bits.  Tensors (any device) or arrays."""
    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    v, t = host(vertices).astype(np.float32), host(indices).astype(np.int64)
    if v.ndim != 2 or v.shape[1] != 3 or t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f"{NAME}.write_obj: vertices must be [V,3] and indices [F,3]")
    if not np.isfinite(v).all():
        raise ValueError(f"{NAME}.write_obj: a position is not finite")
    if t.size and (t.min() < 0 or t.max() >= v.shape[0]):
        raise ValueError(f"{NAME}.write_obj: vertex index out of range")
    with open(path, "w") as f:
        for x, y, z in v.tolist():                                      # Python floats: the float32 values, exactly
            f.write(f"v {x!r} {y!r} {z!r}\n")
        for a, b, c in (t + 1).tolist():
            f.write(f"f {a} {b} {c}\n")
