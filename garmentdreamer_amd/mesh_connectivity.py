"""The device connectivity of a triangle mesh (the tables of include/gd_mesh_remesh.h) and the small host pieces every
module that stands on it needs: the remesher (``mesh_remesh``), the final-mesh post-process (``mesh_simplify``) and the
UV atlas (``texture_atlas``).  No CPU path.

  * ``Connectivity`` / ``build_connectivity(tri, num_vertices, prefix)``   the tables, from sorted 64-bit keys
  * ``mesh_args(prefix, vertices, indices)``                               the argument check: ``(float32 [V,3], int32 [F,3])``
  * ``mesh_struct(vertices, conn)``                                        the ``gd_remesh_mesh`` argument of a launch
  * ``scan`` / ``new_flags`` / ``raise_flags`` / ``empty_i32`` / ``zeros_i32``
  * ``drop_dead_faces(prefix, indices, remap, flags)``                     the tail of a round of collapses

Every function that can raise takes the caller's full message prefix (``"mesh_simplify.decimate_quadric"``), so an error
names the entry the user called."""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Tuple

import torch

from . import _native
from ._launch import launch, require_gpu

MAX_FACES = 1 << 29


class Connectivity(NamedTuple):
    """the tables of include/gd_mesh_remesh.h for one ``tri``, all int32 on the device"""
    tri: torch.Tensor       # [F,3]
    V: int
    F: int
    E: int
    ev: torch.Tensor        # [E,2] (lo, hi), rows sorted
    eh: torch.Tensor        # [E,2] half-edges 3 f + i, the second -1 on the boundary
    fe: torch.Tensor        # [3F] edge of each half-edge
    bnd: torch.Tensor       # [V]
    nbr_ptr: torch.Tensor   # [V+1]
    nbr_idx: torch.Tensor   # [2E]
    vf_ptr: torch.Tensor    # [V+1]
    vf_idx: torch.Tensor    # [3F]


def empty_i32(n, dev):
    return torch.empty(n, dtype=torch.int32, device=dev)


def zeros_i32(n, dev):
    return torch.zeros(n, dtype=torch.int32, device=dev)


def new_flags(dev):
    return torch.zeros(_native.REMESH_FLAGS, dtype=torch.int32, device=dev)


def scan(x: torch.Tensor) -> torch.Tensor:
    """int32 [n+1]: the exclusive scan of ``x`` and its total"""
    out = empty_i32(x.shape[0] + 1, x.device)
    launch("gd_mesh_remesh_scan", x.device, x.shape[0], x, out)
    return out


def raise_flags(prefix: str, flags: List[int]) -> None:
    if flags[_native.REMESH_FLAG_INDEX]:
        raise ValueError(f"{prefix}: vertex index out of range")
    if flags[_native.REMESH_FLAG_REPEATED]:
        raise ValueError(f"{prefix}: a face lists a vertex twice")
    if flags[_native.REMESH_FLAG_NONMANIFOLD]:
        raise ValueError(f"{prefix}: an edge is shared by more than two triangles (non-manifold mesh)")
    if flags[_native.REMESH_FLAG_CAPACITY]:
        raise RuntimeError(f"{prefix}: a table entry or an output position was out of range; nothing was written there")


def mesh_args(prefix: str, vertices, indices) -> Tuple[torch.Tensor, torch.Tensor]:
    v = require_gpu(prefix, "vertices", vertices, torch.float32, 3)
    t = require_gpu(prefix, "indices", indices, None, 3)
    if v.dim() != 2 or t.dim() != 2:
        raise ValueError(f"{prefix}: vertices must be [V,3] and indices [F,3]")
    if t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{prefix}: indices must be int32 or int64")
    if v.shape[0] == 0 or t.shape[0] >= MAX_FACES:
        raise ValueError(f"{prefix}: needs at least one vertex and fewer than 2^29 faces")
    if t.dtype == torch.int64 and t.numel() and int(torch.stack((t.min(), t.max())).abs().max()) >= 1 << 31:
        raise ValueError(f"{prefix}: vertex index out of range")
    return v.detach().contiguous(), t.detach().to(torch.int32).contiguous()


def build_connectivity(tri: torch.Tensor, num_vertices: int, prefix: str = "mesh_remesh.build_connectivity") -> Connectivity:
    """The connectivity of ``tri`` (int32 [F,3] on the GPU, F > 0).  ``ValueError`` for an index out of range, a face that
    lists a vertex twice or an edge with more than two faces; nothing that follows an index has run by then."""
    dev, V, F = tri.device, int(num_vertices), tri.shape[0]
    flags = new_flags(dev)
    hkeys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    ckeys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    launch("gd_mesh_remesh_keys", dev, V, F, tri, hkeys, ckeys, flags)
    skeys, order = torch.sort(hkeys, stable=True)
    sckeys = torch.sort(ckeys).values
    head = empty_i32(3 * F, dev)
    launch("gd_mesh_remesh_heads", dev, 3 * F, skeys, head, flags)
    head_scan = scan(head)
    got = torch.cat((head_scan[-1:], flags)).tolist()                  # the one host read of a build
    E = got[0]
    raise_flags(prefix, got[1:])
    fe, ev, eh = empty_i32(3 * F, dev), empty_i32(2 * E, dev), empty_i32(2 * E, dev)
    ukeys = torch.empty(E, dtype=torch.int64, device=dev)
    rkeys = torch.empty(E, dtype=torch.int64, device=dev)
    bnd = zeros_i32(V, dev)
    launch("gd_mesh_remesh_edge_tables", dev, V, F, E, skeys, order, head_scan, fe, ev, eh, ukeys, rkeys, bnd, flags)
    srkeys = torch.sort(rkeys).values
    nbr_ptr, nbr_idx = empty_i32(V + 1, dev), empty_i32(2 * E, dev)
    vf_ptr, vf_idx = empty_i32(V + 1, dev), empty_i32(3 * F, dev)
    launch("gd_mesh_remesh_vertex_tables", dev, V, F, E, ukeys, srkeys, sckeys, nbr_ptr, nbr_idx, vf_ptr, vf_idx)
    return Connectivity(tri, V, F, E, ev.view(E, 2), eh.view(E, 2), fe, bnd, nbr_ptr, nbr_idx, vf_ptr, vf_idx)


def mesh_struct(v: torch.Tensor, c: Connectivity):
    m = _native.RemeshMesh(c.V, c.F, c.E, v.data_ptr(), c.tri.data_ptr(), c.ev.data_ptr(), c.eh.data_ptr(), c.bnd.data_ptr(),
                           c.nbr_ptr.data_ptr(), c.nbr_idx.data_ptr(), c.vf_ptr.data_ptr(), c.vf_idx.data_ptr())
    return C.byref(m)


def drop_dead_faces(prefix: str, indices: torch.Tensor, remap: torch.Tensor, flags: torch.Tensor):
    """The tail of a round of collapses: relabel ``indices`` (int32 [F,3], F > 0) through ``remap`` (int32 [V]) and drop the
    faces that name a vertex twice afterwards: ``(indices', selected)``, with ``selected`` the round's count in ``flags``;
    ``(indices, 0)``, the input itself, if the round selected nothing.  One host read (the faces left, with ``flags``), and
    one more of the compaction's flags when something was selected."""
    dev, V, F = indices.device, remap.shape[0], indices.shape[0]
    relabelled, alive = torch.empty_like(indices), empty_i32(F, dev)
    launch("gd_mesh_remesh_relabel", dev, V, F, indices, remap, relabelled, alive, flags)
    alive_scan = scan(alive)
    got = torch.cat((alive_scan[-1:], flags)).tolist()
    raise_flags(prefix, got[1:])
    selected = got[1 + _native.REMESH_FLAG_SELECTED]
    if selected == 0:
        return indices, 0
    out = torch.empty((got[0], 3), dtype=torch.int32, device=dev)
    launch("gd_mesh_remesh_compact_faces", dev, F, got[0], relabelled, alive, alive_scan, out, flags)
    raise_flags(prefix, flags.tolist())
    return out, selected
