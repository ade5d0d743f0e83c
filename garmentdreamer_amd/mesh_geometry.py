"""Geometry terms of the mesh deformer (stage 3 of the reference: ``deformer/core/mesh.py``, ``losses/laplacian.py``,
``losses/normal_consistency.py``, ``losses/mask.py``, ``utils/geometry.py``) on the HIP kernels of
``csrc/raster_geometry.hip`` (C-ABI and definitions: include/gd_mesh_geometry.h) -- no CPU path.

  * ``build_geometry(tri)``                       per-mesh host work (numpy): the ``MeshTopology`` of ``mesh_render``, the
                                                  face across each edge, the vertex adjacency as a CSR, ``edges`` and
                                                  ``connected_faces`` as the reference's ``Mesh`` has them
  * ``normals(vertices, geo)``                    ``(face_normals, vertex_normals)`` <- ``Mesh.compute_normals``
  * ``laplacian_loss(vertices | mesh, geo)``      <- ``laplacian_loss`` with ``compute_laplacian_uniform``
  * ``normal_consistency_loss(face_normals | mesh, geo)``  <- ``normal_consistency_loss``
  * ``DeformMesh``                                the reference's ``Mesh`` for a mesh on the GPU
  * ``mask_loss(target_masks, gbuffers)``         the reference's mean of per-view MSE, plain torch

The three ops are autograd functions.  The reference states them as gathers, ``index_add`` and a sparse ``mm`` whose
backwards scatter with floating-point atomics; here every sum has a fixed order (a vertex gathers its corners or its
neighbours, a loss is reduced in a fixed tree), so a rerun is bit-identical, and nothing synchronises with the host.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _native
from ._launch import launch, require_gpu, scratch
from ._mesh_ops import MeshTopology, build_topology, edge_groups, host_triangles


class MeshGeometry(NamedTuple):
    topology: MeshTopology          # opp / corner_ptr / corner_idx of mesh_render.build_topology
    tri: torch.Tensor               # int32 [F,3]
    face_nbr: torch.Tensor          # int32 [F,3]: face across edge i (between corners i+1, i+2), -1 unless exactly 2 share it
    nbr_ptr: torch.Tensor           # int32 [V+1]
    nbr_idx: torch.Tensor           # int32 [2E']: the vertices sharing an edge with each vertex, ascending
    edges: torch.Tensor             # int64 [E,2]: each row sorted, rows unique and sorted (the reference's mesh.edges)
    connected_faces: torch.Tensor   # int64 [P,2]: f < g for every edge shared by exactly the faces f and g
    num_vertices: int
    num_pairs: int


def build_geometry(tri, num_vertices: Optional[int] = None, device=None) -> MeshGeometry:
    """Connectivity of ``tri`` (tensor or array [F,3]), computed once per mesh on the host with numpy and uploaded to
    ``device`` (default: the device of ``tri`` if it is a tensor, else the CPU).  Raises ``ValueError`` if an edge is shared
    by more than two triangles (the reference asserts the same).  Two faces that share three edges (duplicates) form three
    pairs, as in the reference.  A face that lists a vertex twice is outside the definitions: it forms no pair with itself
    and its edge (v, v), though listed in ``edges``, makes no vertex its own neighbour."""
    t, nv, device = host_triangles(tri, num_vertices, device)
    nf = t.shape[0]
    topology = build_topology(t, num_vertices=nv, device=device)       # checks the index range
    lo, hi, order, start, count = edge_groups(t, nv)
    if nf and count.max() > 2:
        raise ValueError("build_geometry: an edge is shared by more than two triangles (non-manifold mesh)")
    edges = np.stack((lo[order[start]], hi[order[start]]), axis=1).reshape(-1, 2)
    first = start[count == 2]
    a, b = order[first], order[first + 1]
    keep = (a // 3) != (b // 3)
    a, b = a[keep], b[keep]
    face_nbr = np.full(3 * nf, -1, dtype=np.int32)
    face_nbr[a], face_nbr[b] = b // 3, a // 3
    pairs = np.stack((np.minimum(a // 3, b // 3), np.maximum(a // 3, b // 3)), axis=1).reshape(-1, 2)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    proper = edges[edges[:, 0] != edges[:, 1]]
    src = np.concatenate((proper[:, 0], proper[:, 1]))
    dst = np.concatenate((proper[:, 1], proper[:, 0]))
    by = np.lexsort((dst, src))
    nbr_ptr = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=nv), out=nbr_ptr[1:])
    dev = torch.device("cpu") if device is None else torch.device(device)

    def up(x, dtype):
        return torch.from_numpy(np.ascontiguousarray(x.astype(dtype))).to(dev)

    return MeshGeometry(topology, up(t, np.int32), up(face_nbr.reshape(nf, 3), np.int32), up(nbr_ptr, np.int32),
                        up(dst[by], np.int32), up(edges, np.int64), up(pairs, np.int64), nv, int(pairs.shape[0]))


def _geometry(name: str, geo: MeshGeometry, V: Optional[int], F: Optional[int]) -> MeshGeometry:
    if not isinstance(geo, MeshGeometry):
        raise TypeError(f"{name}: geo must be the MeshGeometry of build_geometry")
    if not geo.tri.is_cuda or (V is not None and geo.num_vertices != V) or (F is not None and geo.tri.shape[0] != F):
        raise ValueError(f"{name}: geo does not belong to this mesh (or is not on the GPU)")
    return geo


class _Normals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, geo):
        dev = vertices.device
        V, nf = vertices.shape[0], geo.tri.shape[0]
        fn = torch.empty((nf, 3), dtype=torch.float32, device=dev)
        vn = torch.empty((V, 3), dtype=torch.float32, device=dev)
        length = torch.empty(V, dtype=torch.float32, device=dev)
        launch("gd_mesh_normals_forward", dev, V, nf, vertices, geo.tri, geo.topology.corner_ptr,
               geo.topology.corner_idx, fn, vn, length)
        ctx.save_for_backward(vertices, vn, length)
        ctx.geo = geo
        ctx.set_materialize_grads(False)
        return fn, vn

    @staticmethod
    def backward(ctx, dfn, dvn):
        vertices, vn, length = ctx.saved_tensors
        geo, topo = ctx.geo, ctx.geo.topology
        dev = vertices.device
        V, nf = vertices.shape[0], geo.tri.shape[0]
        if dfn is None and dvn is None:
            return None, None
        dfn = None if dfn is None else dfn.contiguous()
        dvn = None if dvn is None else dvn.contiguous()
        dverts = torch.empty((V, 3), dtype=torch.float32, device=dev)
        launch("gd_mesh_normals_backward", dev, V, nf, vertices, geo.tri, topo.corner_ptr, topo.corner_idx, vn, length,
               dvn, dfn, dverts, scratch(_native.lib().gd_mesh_normals_backward_scratch_bytes(nf), dev))
        return dverts, None


def normals(vertices: torch.Tensor, geo: MeshGeometry):
    """``(face_normals [F,3], vertex_normals [V,3])`` of ``vertices`` (float32 [V,3]) as ``Mesh.compute_normals`` defines
    them: the normalised cross product per face, the normalised sum of the faces around a vertex (0 for a vertex no face
    uses), both with ``torch.nn.functional.normalize``'s 1e-12.  Differentiable in ``vertices`` through either output."""
    require_gpu("normals", "vertices", vertices, torch.float32, 3)
    if vertices.dim() != 2:
        raise ValueError("normals: vertices must be [V,3]")
    geo = _geometry("normals", geo, vertices.shape[0], None)
    return _Normals.apply(vertices.contiguous(), geo)


class _Laplacian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, geo):
        dev = vertices.device
        V = vertices.shape[0]
        delta = torch.empty((V, 3), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        launch("gd_mesh_laplacian_forward", dev, V, geo.nbr_idx.shape[0], vertices, geo.nbr_ptr, geo.nbr_idx, delta, loss,
               scratch(_native.lib().gd_mesh_loss_scratch_bytes(V), dev))
        ctx.save_for_backward(delta)
        ctx.geo = geo
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (delta,) = ctx.saved_tensors
        geo = ctx.geo
        V = delta.shape[0]
        dverts = torch.empty((V, 3), dtype=torch.float32, device=delta.device)
        launch("gd_mesh_laplacian_backward", delta.device, V, geo.nbr_idx.shape[0], geo.nbr_ptr, geo.nbr_idx, delta,
               dloss.contiguous(), dverts)
        return dverts, None


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fn, geo):
        dev = fn.device
        nf = fn.shape[0]
        loss = torch.empty((), dtype=torch.float32, device=dev)
        launch("gd_mesh_normal_consistency_forward", dev, nf, geo.num_pairs, fn, geo.face_nbr, loss,
               scratch(_native.lib().gd_mesh_loss_scratch_bytes(nf), dev))
        ctx.save_for_backward(fn)
        ctx.geo = geo
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (fn,) = ctx.saved_tensors
        geo = ctx.geo
        dev = fn.device
        nf = fn.shape[0]
        dfn = torch.zeros((nf, 3), dtype=torch.float32, device=dev) if nf == 0 else \
            torch.empty((nf, 3), dtype=torch.float32, device=dev)
        launch("gd_mesh_normal_consistency_backward", dev, nf, geo.num_pairs, fn, geo.face_nbr, dloss.contiguous(), dfn)
        return dfn, None


class DeformMesh:
    """The reference's ``Mesh`` (deformer/core/mesh.py) for a mesh on the GPU: ``vertices`` float32 [V,3], ``indices``
    int64 [F,3], ``face_normals`` and ``vertex_normals`` computed at construction and part of the autograd graph of
    ``vertices``, ``edges`` / ``connected_faces`` from the ``MeshGeometry`` (built here if none is passed: a host pass
    over the mesh), which ``with_vertices`` shares."""

    def __init__(self, vertices: torch.Tensor, indices: torch.Tensor, geometry: Optional[MeshGeometry] = None):
        require_gpu("DeformMesh", "vertices", vertices, torch.float32, 3)
        require_gpu("DeformMesh", "indices", indices)
        self.device = vertices.device
        self.vertices = vertices
        self.indices = indices.to(torch.int64)
        if geometry is None:
            geometry = build_geometry(indices, num_vertices=vertices.shape[0], device=vertices.device)
        self.geometry = _geometry("DeformMesh", geometry, vertices.shape[0], indices.shape[0])
        self.face_normals, self.vertex_normals = normals(vertices, self.geometry)

    @property
    def edges(self) -> torch.Tensor:
        return self.geometry.edges

    @property
    def connected_faces(self) -> torch.Tensor:
        return self.geometry.connected_faces

    def with_vertices(self, vertices: torch.Tensor) -> "DeformMesh":
        """A mesh with the same connectivity and other vertex positions (its normals are computed anew)."""
        if len(vertices) != len(self.vertices):
            raise ValueError("with_vertices: one row per vertex of this mesh")
        return DeformMesh(vertices, self.indices, self.geometry)

    def detach(self) -> "DeformMesh":
        mesh = DeformMesh.__new__(DeformMesh)
        mesh.device, mesh.indices, mesh.geometry = self.device, self.indices, self.geometry
        mesh.vertices = self.vertices.detach()
        mesh.face_normals, mesh.vertex_normals = self.face_normals.detach(), self.vertex_normals.detach()
        return mesh


def laplacian_loss(vertices: Union[torch.Tensor, DeformMesh], geo: Optional[MeshGeometry] = None) -> torch.Tensor:
    """Mean over the vertices of ``|delta_i|^2``, ``delta_i`` = the mean of the edge neighbours minus the vertex
    (``L.mm(V).norm(dim=1)**2).mean()`` with the reference's uniform Laplacian).  Takes ``vertices`` float32 [V,3] with
    ``geo``, or a ``DeformMesh``.  A 0-dim tensor on the device."""
    if isinstance(vertices, DeformMesh):
        vertices, geo = vertices.vertices, vertices.geometry
    require_gpu("laplacian_loss", "vertices", vertices, torch.float32, 3)
    if vertices.dim() != 2:
        raise ValueError("laplacian_loss: vertices must be [V,3]")
    return _Laplacian.apply(vertices.contiguous(), _geometry("laplacian_loss", geo, vertices.shape[0], None))


def normal_consistency_loss(face_normals: Union[torch.Tensor, DeformMesh],
                            geo: Optional[MeshGeometry] = None) -> torch.Tensor:
    """Mean over ``connected_faces`` of ``(1 - cosine_similarity(fn_f, fn_g))^2`` (eps 1e-8).  Takes ``face_normals``
    float32 [F,3] with ``geo``, or a ``DeformMesh``.  A mesh without a pair gives 0 (the reference: NaN)."""
    if isinstance(face_normals, DeformMesh):
        face_normals, geo = face_normals.face_normals, face_normals.geometry
    require_gpu("normal_consistency_loss", "face_normals", face_normals, torch.float32, 3)
    if face_normals.dim() != 2:
        raise ValueError("normal_consistency_loss: face_normals must be [F,3]")
    geo = _geometry("normal_consistency_loss", geo, None, face_normals.shape[0])
    return _NormalConsistency.apply(face_normals.contiguous(), geo)


def mask_loss(target_masks: Sequence[torch.Tensor], gbuffers: Sequence[dict]) -> torch.Tensor:
    """The reference's ``mask_loss`` (losses/mask.py): the mean over the views of the MSE between the view's mask and the
    rendered ``gbuffer["mask"]``.  Plain torch."""
    loss = 0.0
    for target, gbuffer in zip(target_masks, gbuffers):
        loss = loss + torch.nn.functional.mse_loss(gbuffer["mask"], target)
    return loss / len(gbuffers)
