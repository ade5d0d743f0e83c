"""Initial point cloud of the Gaussian scene from a garment template mesh -- the host-side mirror of
``GaussianDreamer.template`` / ``add_points`` / ``pcb``
(Garment_3DGS/threestudio/systems/GaussianDreamer.py:115-177), without ``open3d``:

  * ``load_obj``            ``v`` / ``f`` lines of a Wavefront OBJ (numpy);
  * ``load_obj_uv``         the same with the ``vt`` lines and ``a/b`` corners (what ``texture_bake`` writes);
  * ``sample_surface``      area-uniform surface samples, seeded, float64 (numpy; init-time work, not a hot path);
  * ``shell_search``        nearest sample of every query within a fixed radius: the HIP kernels of
                            ``csrc/raster_template.hip`` (``gd_scene_shell_search``, include/gd_scene.h) -- no CPU path.
                            The reference asks a KD-tree once per candidate from a Python loop;
  * ``template_point_cloud``  samples + the "shell" of box-uniform candidates within ``deviation`` of a sample (what
                            gives the cloth its thickness), colours, scaled by ``radius * scale``.

``GaussianModel.create_from_template`` feeds the result to ``create_from_pcd``.
"""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import numpy as np
import torch

from . import _native
from ._launch import launch, scratch
from .scene import SH_C0


def SH2RGB(sh):
    """utils/sh_utils.py:117-118"""
    return sh * SH_C0 + 0.5


def load_obj(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(vertices float64 [V,3], faces int64 [F,3]) from the ``v`` and ``f`` lines of an OBJ file.  A face corner may be
    written ``a``, ``a/b``, ``a//c`` or ``a/b/c`` (only ``a`` is used); a negative index counts back from the vertices
    read so far; a polygon becomes a fan from its first corner.  ``ValueError`` for an index out of range or a file
    without faces."""
    verts, faces = [], []
    with open(path, "r") as f:
        for lineno, line in enumerate(f, 1):
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError(f"{path}:{lineno}: a vertex needs three coordinates")
                verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
            elif tok[0] == "f":
                corners = []
                for t in tok[1:]:
                    i = int(t.split("/", 1)[0])
                    if i < 0:
                        i += len(verts)
                        if i < 0:
                            raise ValueError(f"{path}:{lineno}: relative vertex index {t} out of range")
                    elif i == 0:
                        raise ValueError(f"{path}:{lineno}: vertex index 0 (OBJ indices start at 1)")
                    else:
                        i -= 1
                    corners.append(i)
                if len(corners) < 3:
                    raise ValueError(f"{path}:{lineno}: a face needs at least three corners")
                faces += [(corners[0], corners[k], corners[k + 1]) for k in range(1, len(corners) - 1)]
    if not faces:
        raise ValueError(f"{path}: no faces")
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    fa = np.asarray(faces, dtype=np.int64)
    if fa.max() >= v.shape[0]:
        raise ValueError(f"{path}: vertex index {int(fa.max()) + 1} out of range ({v.shape[0]} vertices)")
    return v, fa


def load_obj_uv(path: str):
    """``load_obj`` plus the texture coordinates: (v float64 [V,3], f int64 [F,3], vt float64 [T,2], ft int64 [F,3]) from
    the ``v``, ``vt`` and ``f`` lines; a corner is ``a/b`` or ``a/b/c``.  ``vt`` and ``ft`` are ``None`` when any corner of
    any face has no texture index (``a`` or ``a//c``).  Polygons, negative indices (relative to the ``v`` / ``vt`` read so
    far) and the errors follow ``load_obj``; ``vt`` is returned as written (``write_textured_obj`` writes ``1 - v``)."""
    verts, coords, faces, tfaces = [], [], [], []
    textured = True

    def index(tok, t, count, lineno, what):
        i = int(t)
        if i < 0:
            i += count
            if i < 0:
                raise ValueError(f"{path}:{lineno}: relative {what} index {tok} out of range")
            return i
        if i == 0:
            raise ValueError(f"{path}:{lineno}: {what} index 0 (OBJ indices start at 1)")
        return i - 1

    with open(path, "r") as f:
        for lineno, line in enumerate(f, 1):
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError(f"{path}:{lineno}: a vertex needs three coordinates")
                verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
            elif tok[0] == "vt":
                if len(tok) < 3:
                    raise ValueError(f"{path}:{lineno}: a texture coordinate needs two components")
                coords.append((float(tok[1]), float(tok[2])))
            elif tok[0] == "f":
                corners, tcorners = [], []
                for t in tok[1:]:
                    parts = t.split("/")
                    corners.append(index(t, parts[0], len(verts), lineno, "vertex"))
                    if len(parts) > 1 and parts[1]:
                        tcorners.append(index(t, parts[1], len(coords), lineno, "texture"))
                    else:
                        textured = False
                if len(corners) < 3:
                    raise ValueError(f"{path}:{lineno}: a face needs at least three corners")
                faces += [(corners[0], corners[k], corners[k + 1]) for k in range(1, len(corners) - 1)]
                if textured:
                    tfaces += [(tcorners[0], tcorners[k], tcorners[k + 1]) for k in range(1, len(tcorners) - 1)]
    if not faces:
        raise ValueError(f"{path}: no faces")
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    fa = np.asarray(faces, dtype=np.int64)
    if fa.max() >= v.shape[0]:
        raise ValueError(f"{path}: vertex index {int(fa.max()) + 1} out of range ({v.shape[0]} vertices)")
    if not textured:
        return v, fa, None, None
    vt = np.asarray(coords, dtype=np.float64).reshape(-1, 2)
    ft = np.asarray(tfaces, dtype=np.int64)
    if ft.max() >= vt.shape[0]:
        raise ValueError(f"{path}: texture index {int(ft.max()) + 1} out of range ({vt.shape[0]} texture coordinates)")
    return v, fa, vt, ft


def sample_surface(vertices, faces, n: int, seed: int) -> np.ndarray:
    """``n`` points uniform in area on the mesh, float64 [n,3].  One ``RandomState(seed)`` draw of ``random((n, 3))``:
    column 0 picks the triangle through the cumulative areas (a zero-area triangle is never chosen), columns 1 and 2
    are the square-root barycentric map.  numpy's global generator is not touched."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cdf = np.cumsum(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1))
    total = cdf[-1]
    if not (total > 0.0 and np.isfinite(total)):
        raise ValueError("sample_surface: the mesh has no area")
    r = np.random.RandomState(seed).random((n, 3))
    tri = np.minimum(np.searchsorted(cdf, r[:, 0] * total, side="right"), f.shape[0] - 1)
    s = np.sqrt(r[:, 1])
    w0, w1, w2 = 1.0 - s, s * (1.0 - r[:, 2]), s * r[:, 2]
    return w0[:, None] * a[tri] + w1[:, None] * b[tri] + w2[:, None] * c[tri]


def shell_search(samples: torch.Tensor, queries: torch.Tensor, radius: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(nearest int32 [Q], dist2 float32 [Q]): for every query the index of the nearest sample if it is closer than
    ``radius`` (fp32: ``d2 < fl(radius * radius)``, lowest index on equal ``d2``), else -1, and the smallest squared
    distance found in the cells around the query (+inf if there was none).  float32 CUDA tensors [S,3] / [Q,3]; runs on
    the current stream (one host read of the samples' bounding box)."""
    if not samples.is_cuda or not queries.is_cuda:
        raise RuntimeError("shell_search: the HIP kernels have no CPU path (samples and queries must be on the GPU)")
    if samples.dtype != torch.float32 or queries.dtype != torch.float32:
        raise TypeError("shell_search: samples and queries must be float32")
    if samples.dim() != 2 or samples.shape[1] != 3 or queries.dim() != 2 or queries.shape[1] != 3:
        raise ValueError("shell_search: samples and queries must be [N,3]")
    if queries.device != samples.device:
        raise ValueError("shell_search: samples and queries must be on one device")
    dev = samples.device
    smp, qry = samples.detach().contiguous(), queries.detach().contiguous()
    S, Q = smp.shape[0], qry.shape[0]
    box = torch.stack((smp.min(dim=0).values, smp.max(dim=0).values)).cpu().numpy() if S else np.zeros((2, 3), np.float32)
    lo, hi = (C.c_float * 3)(*box[0].tolist()), (C.c_float * 3)(*box[1].tolist())
    L = _native.lib()
    edge, dims = C.c_float(0), (C.c_int * 3)()
    _native.checked("gd_scene_shell_grid", L.gd_scene_shell_grid(lo, hi, float(radius), C.byref(edge), dims))
    nearest = torch.empty(Q, dtype=torch.int32, device=dev)
    dist2 = torch.empty(Q, dtype=torch.float32, device=dev)
    launch("gd_scene_shell_search", dev, S, smp, Q, qry, lo, hi, float(radius), nearest, dist2,
           scratch(L.gd_scene_shell_scratch_bytes(S, dims[0] * dims[1] * dims[2]), dev))
    return nearest, dist2


def template_point_cloud(mesh_path: str, num_pts: int = 50000, num_pts_space: int = 500000, deviation: float = 0.01,
                         radius: float = 4.0, scale: float = 0.4, seed: int = 0, device="cuda"):
    """(points float32 [P,3], colors float32 [P,3], bound): the reference's ``pcb()`` point cloud on ``device``.

    1. ``num_pts`` surface samples of the mesh, axes permuted (z, x, y) as ``template()`` does;
    2. their colours ``SH2RGB(u / 255)``, ``u`` from ``RandomState(seed + 1)`` (the reference's are unseeded);
    3. ``num_pts_space`` candidates uniform in the samples' bounding box from ``RandomState(0)`` (the reference's
       ``np.random.seed(0)`` stream, without touching the global generator);
    4. ``shell_search`` of the float32 candidates against the float32 samples with ``radius = deviation``;
    5. the accepted candidates, in candidate order;
    6. their colours: the nearest sample's plus ``0.2 *`` the next ``(n_accepted, 3)`` draws of the same stream;
    7. ``[accepted ; samples] * bound`` and ``[shell colours ; sample colours]`` (not clamped), ``bound = radius * scale``.
    """
    dev = torch.device(device)
    vertices, faces = load_obj(mesh_path)
    coords = sample_surface(vertices, faces, num_pts, seed)[:, [2, 0, 1]]
    rgb = SH2RGB(np.random.RandomState(seed + 1).random((num_pts, 3)) / 255.0)
    stream = np.random.RandomState(0)
    cand = stream.uniform(low=coords.min(axis=0), high=coords.max(axis=0), size=(num_pts_space, 3))
    coords32 = torch.from_numpy(coords.astype(np.float32)).to(dev)
    cand32 = torch.from_numpy(cand.astype(np.float32)).to(dev)
    nearest, _ = shell_search(coords32, cand32, deviation)
    keep = nearest >= 0
    accepted = cand32[keep]
    near = nearest[keep].cpu().numpy().astype(np.int64)
    shell_rgb = rgb[near] + 0.2 * stream.random((near.shape[0], 3))
    bound = radius * scale
    points = torch.cat((accepted, coords32), dim=0) * bound
    colors = torch.from_numpy(np.concatenate((shell_rgb, rgb), axis=0).astype(np.float32)).to(dev)
    return points, colors, bound
