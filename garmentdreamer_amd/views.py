"""Reading the captured views from disk: what stage 3 (``Garment_Deformer_NeTF/deformer/utils/io.py:read_views``,
``deformer/core/view.py``, ``deformer/modules/space_normalization.py``, ``deformer/utils/geometry.py:AABB``,
``deformer/core/renderer.py:set_near_far``, ``deformer/modules/view_sampler.py``, ``deformer/tools/adjust_mesh.py``) and
stage 4 (``netf/view_core/view.py``) make of ``gs_rendered_rgba/*.png``, ``estimated_normals/*.png`` and ``cameras.json``,
the files ``export.dump_test_view`` / ``save_cameras_json`` write.

The images have no CPU path: the files are parsed and inflated on the host (``export.read_png_stream``, a thread pool of a
fixed size), uploaded once per batch of equal geometry, unfiltered by ``gd_views_png_unfilter`` and turned into float
images by ``gd_views_unpack`` / ``gd_views_unpack_rgba`` (include/gd_views.h).  The cameras are a few 4x4 matrices per
view and stay on the host, in float64 until they are handed on."""
from __future__ import annotations

import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from ._launch import launch
from .export import read_png_stream, undefined_row_filter
from .mesh_deform import GBufferRenderer

NAME = "views"
RGB_DIRECTORY, NORMAL_DIRECTORY, CAMERAS_FILE = "gs_rendered_rgba", "estimated_normals", "cameras.json"


# ---- the kernels ------------------------------------------------------------------------------------------------------

def _bytes_on_gpu(what: str, t, shape_hint: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{NAME}: {what} must be a uint8 tensor on the GPU (the HIP kernels have no CPU path)")
    if t.dtype != torch.uint8:
        raise ValueError(f"{NAME}: {what} must be uint8 {shape_hint}")
    return t.contiguous()


def _aligned(t: torch.Tensor, to: int) -> torch.Tensor:
    return t if t.data_ptr() % to == 0 else t.clone()


def png_unfilter(filtered, B: int, H: int, W: int, bpp: int) -> torch.Tensor:
    """uint8 [B,H,W,bpp] of ``filtered``: uint8 on the GPU, ``B`` inflated PNG streams of ``H`` rows of ``1 + W bpp`` bytes."""
    f = _bytes_on_gpu("filtered", filtered, "[B H (1 + W bpp)]").reshape(-1)
    B, H, W, bpp = int(B), int(H), int(W), int(bpp)
    if min(B, H, W) < 1 or bpp not in (3, 4) or f.numel() != B * H * (1 + W * bpp):
        raise ValueError(f"{NAME}: filtered must hold B H (1 + W bpp) bytes with B, H, W >= 1 and bpp 3 or 4")
    f = _aligned(f, 4)
    out = torch.empty((B, H, W, bpp), dtype=torch.uint8, device=f.device)
    launch("gd_views_png_unfilter", f.device, f, out, B, H, W, bpp)
    return out


def _image_bytes(what: str, t, channels: Sequence[int]) -> torch.Tensor:
    t = _bytes_on_gpu(what, t, "[H,W,C]")
    if t.dim() != 3 or t.shape[2] not in channels or t.numel() == 0:
        raise ValueError(f"{NAME}: {what} must be uint8 [H,W,{' or '.join(str(c) for c in channels)}]")
    return _aligned(t, 16)


def unpack_view(normal_rgba, rgb) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(``normal`` [H,W,3], ``mask`` [H,W,1], ``rgb`` [H,W,3]) float32 of a view's two byte images (``View.load``):
    ``x = byte / 255``, the mask is the alpha of the normal image, ``normal = ((x 2 - 1) (1, -1, 1) + 1) / 2``."""
    n = _image_bytes("normal_rgba", normal_rgba, (4,))
    c = _image_bytes("rgb", rgb, (3, 4))
    if c.device != n.device or c.shape[:2] != n.shape[:2]:
        raise ValueError(f"{NAME}: normal_rgba and rgb must have one resolution and one device")
    H, W = n.shape[:2]
    normal = torch.empty((H, W, 3), dtype=torch.float32, device=n.device)
    mask = torch.empty((H, W, 1), dtype=torch.float32, device=n.device)
    out = torch.empty((H, W, 3), dtype=torch.float32, device=n.device)
    launch("gd_views_unpack", n.device, n, c, c.shape[2], normal, mask, out, H, W)
    return normal, mask, out


def unpack_rgba(rgba) -> Tuple[torch.Tensor, torch.Tensor]:
    """(``rgb`` [H,W,3], ``mask`` [H,W,1]) float32 of one RGBA byte image (stage 4's ``View.load``)."""
    c = _image_bytes("rgba", rgba, (4,))
    H, W = c.shape[:2]
    out = torch.empty((H, W, 3), dtype=torch.float32, device=c.device)
    mask = torch.empty((H, W, 1), dtype=torch.float32, device=c.device)
    launch("gd_views_unpack_rgba", c.device, c, out, mask, H, W)
    return out, mask


# ---- PNG files --------------------------------------------------------------------------------------------------------

def _inflate(path: str):
    """``read_png_stream`` plus the check of the row types, which the kernel does not repeat"""
    W, H, bpp, raw = read_png_stream(path)
    if max(H, W) > _native.VIEWS_MAX_SIDE:
        raise ValueError(f"{path}: {W} x {H} is larger than {_native.VIEWS_MAX_SIDE} on a side")
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + W * bpp)
    kinds = rows[:, 0]
    if kinds.max() > 4:
        raise undefined_row_filter(path, int(kinds[kinds > 4][0]))
    return (H, W, bpp), rows


class _Clock:
    """seconds per phase into ``timings`` when one is given (each phase then waits for the GPU); nothing otherwise"""

    def __init__(self, timings: Optional[Dict[str, float]], device):
        self.timings, self.device = timings, device
        self.at = time.perf_counter()

    def lap(self, phase: str, gpu: bool = False) -> None:
        if self.timings is None:
            return
        if gpu:
            torch.cuda.synchronize(self.device)
        now = time.perf_counter()
        self.timings[phase] = self.timings.get(phase, 0.0) + (now - self.at)
        self.at = now


def _inflate_all(paths: Sequence[str], workers: int, device, clock: "_Clock") -> list:
    """``_inflate`` of every path on ``workers`` threads (a fixed count: inflating releases the GIL)"""
    workers = int(workers)
    if workers < 1:
        raise ValueError(f"{NAME}: workers must be at least 1")
    if torch.device(device).type != "cuda":
        raise ValueError(f"{NAME}: device must be a GPU (the images have no CPU path)")
    with ThreadPoolExecutor(max_workers=workers) as pool:
        streams = list(pool.map(_inflate, [os.fspath(p) for p in paths]))
    clock.lap("inflate")
    return streams


def _unfilter_group(rows: Sequence[np.ndarray], geometry, device, clock: "_Clock") -> torch.Tensor:
    """uint8 [B,H,W,bpp] of B streams of one geometry: one pinned buffer, one upload, one launch"""
    H, W, bpp = geometry
    staging = torch.empty(len(rows) * H * (1 + W * bpp), dtype=torch.uint8).pin_memory()
    host = staging.numpy().reshape(len(rows), H, 1 + W * bpp)
    for k, stream in enumerate(rows):
        host[k] = stream
    filtered = staging.to(device, non_blocking=True)
    clock.lap("upload", gpu=True)
    images = png_unfilter(filtered, len(rows), H, W, bpp)
    clock.lap("unfilter", gpu=True)
    return images


def _unfilter_all(streams: list, device, clock: "_Clock") -> List[torch.Tensor]:
    """One uint8 [H,W,bpp] GPU tensor per stream of ``_inflate_all``, the streams grouped by geometry"""
    groups: Dict[tuple, List[int]] = {}
    for i, (geometry, _) in enumerate(streams):
        groups.setdefault(geometry, []).append(i)
    out: List[Optional[torch.Tensor]] = [None] * len(streams)
    for geometry, members in groups.items():
        images = _unfilter_group([streams[i][1] for i in members], geometry, device, clock)
        for k, i in enumerate(members):
            out[i] = images[k]
    return out


def decode_png_batch(paths: Sequence[str], workers: int = 8, device="cuda", timings=None) -> torch.Tensor:
    """uint8 [B,H,W,bpp] on the GPU of ``B`` PNG files of one geometry.  Refuses what ``export.load_image_rgb`` refuses, with
    its messages, and a row filter type above 4.  ``workers``: the threads that inflate."""
    if len(paths) == 0:
        raise ValueError(f"{NAME}: decode_png_batch needs at least one path")
    clock = _Clock(timings, torch.device(device))
    streams = _inflate_all(paths, workers, device, clock)
    for path, (geometry, _) in zip(paths, streams):
        if geometry != streams[0][0]:
            raise ValueError(f"{os.fspath(path)}: (H, W, bpp) = {geometry} differs from {streams[0][0]} of "
                             f"{os.fspath(paths[0])}: a batch has one geometry")
    return _unfilter_group([rows for _, rows in streams], streams[0][0], device, clock)


# ---- cameras ----------------------------------------------------------------------------------------------------------

def _intrinsics(record) -> np.ndarray:
    return np.array([[record["fx"], 0, record["width"] / 2], [0, record["fy"], record["height"] / 2], [0, 0, 1]],
                    dtype=np.float64)


def c2w_from_record(record) -> Tuple[np.ndarray, np.ndarray]:
    """(``C2W`` [4,4], ``K`` [3,3]) float64 of one ``cameras.json`` record as stage 4 takes it: rotation and position as
    they are written, ``cx = width / 2``, ``cy = height / 2``."""
    c2w = np.zeros((4, 4), dtype=np.float64)
    c2w[:3, :3] = np.array(record["rotation"], dtype=np.float64)
    c2w[:3, 3] = np.array(record["position"], dtype=np.float64)
    c2w[3, 3] = 1
    return c2w, _intrinsics(record)


def camera_from_record(record) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(``K`` [3,3], ``R`` [3,3], ``t`` [3]) float64 of one ``cameras.json`` record as the deformer takes it (``View.load``,
    mode 1), operation for operation: column 0 negated; the position's y, and of row 1 the entries of columns 0 and 2,
    negated; column 1 rebuilt as the normalised cross product of columns 2 and 0; column 2 negated; ``[R | t]`` from the
    inverse of the 4x4 ``C2W``."""
    position = np.array(record["position"], dtype=np.float64)
    rotation = np.array(record["rotation"], dtype=np.float64)
    rotation[:, 0] *= -1
    position[1] = -position[1]
    rotation[1, 0] = -rotation[1, 0]
    rotation[1, 2] = -rotation[1, 2]
    rotation[:, 1] = np.cross(rotation[:, 2], rotation[:, 0])
    rotation[:, 1] = rotation[:, 1] / np.linalg.norm(rotation[:, 1])
    rotation[:, 2] *= -1
    c2w = np.zeros((4, 4), dtype=np.float64)
    c2w[:3, :3] = rotation
    c2w[:3, 3] = position
    c2w[3, 3] = 1
    w2c = np.linalg.inv(c2w)
    return _intrinsics(record), w2c[:3, :3], w2c[:3, 3]


def normalize_camera(K, R, t, A) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The camera ``K (R x + t)`` after the space moved by ``A``: ``View.transform`` for an ``A`` that is a uniform scale
    ``s > 0`` and a translation, in float64.  The reference composes ``P = K [R | t] A^-1`` and decomposes it again; for
    such an ``A`` that gives ``K' = K / K[2,2]``, ``R' = R``, the centre ``c' = A c`` and ``t' = -R c'``.  Any other ``A``
    raises ``ValueError``."""
    A = np.asarray(A, dtype=np.float64)
    if A.shape != (4, 4):
        raise ValueError(f"{NAME}: A must be [4,4]")
    s = A[0, 0]
    if not (s > 0 and np.isfinite(A).all()) or not np.array_equal(A[:3, :3], s * np.eye(3)) \
            or not np.array_equal(A[3], [0, 0, 0, 1]):
        raise ValueError(f"{NAME}: A must be a uniform scale s > 0 and a translation (the closed form of View.transform "
                         "holds for no other map)")
    K, R, t = (np.asarray(x, dtype=np.float64) for x in (K, R, t))
    center = np.linalg.solve(R, -t)        # the point with R c + t = 0 (the null vector of P), not -R^T t: R comes from float32
    moved = s * center + A[:3, 3]          # records and is orthogonal to 1e-7 only
    return K / K[2, 2], R.copy(), -R @ moved


class View:
    """A camera and, when it was read with them, its images.  ``normal`` [H,W,3], ``mask`` [H,W,1] and ``rgb`` [H,W,3] are
    float32 on the GPU (``None`` for a view of ``read_cameras``); ``K`` [3,3], ``R`` [3,3], ``t`` [3] and ``center`` [3] are
    float32 host tensors, the casts of the float64 ``camera64`` that ``SpaceNormalization`` works on."""

    def __init__(self, K, R, t, resolution, normal=None, mask=None, rgb=None, name: str = ""):
        self.resolution = (int(resolution[0]), int(resolution[1]))          # (H, W)
        self.normal, self.mask, self.rgb, self.name = normal, mask, rgb, name
        self.set_camera(K, R, t)

    def set_camera(self, K, R, t) -> None:
        self.camera64 = tuple(np.array(x, dtype=np.float64) for x in (K, R, t))
        self.K, self.R, self.t = (torch.from_numpy(x.astype(np.float32)) for x in self.camera64)

    @property
    def center(self) -> torch.Tensor:
        return -self.R.t() @ self.t

    def project(self, points: torch.Tensor, depth_as_distance: bool = False) -> torch.Tensor:
        """[..., 3]: the pixel coordinates of ``points`` [..., 3] under ``x = K (R X + t)`` and their depth, the camera-space
        z or, with ``depth_as_distance``, the distance to the camera's centre.  On the device and in the type of ``points``."""
        K, R, t = (x.to(device=points.device, dtype=points.dtype) for x in (self.K, self.R, self.t))
        points_c = points @ R.t() + t
        pixels = points_c @ K.t()
        pixels = pixels[..., :2] / pixels[..., 2:]
        depths = torch.norm(points_c, p=2, dim=-1, keepdim=True) if depth_as_distance else points_c[..., 2:]
        return torch.cat([pixels, depths], dim=-1)


def _listing(directory: str, sub: str) -> List[str]:
    folder = os.path.join(directory, sub)
    if not os.path.isdir(folder):
        raise ValueError(f"{folder}: no such directory of views")
    names = [n for n in os.listdir(folder) if n.endswith(".png") and os.path.isfile(os.path.join(folder, n))]
    for n in names:
        if not n[:-4].isdigit():
            raise ValueError(f"{os.path.join(folder, n)}: the name of a view must be its integer index")
    return [os.path.join(folder, n) for n in sorted(names, key=lambda n: int(n[:-4]))]


def _stem(path: str) -> str:
    return os.path.basename(path)[:-4]


def _records(directory: str) -> List[dict]:
    path = os.path.join(directory, CAMERAS_FILE)
    if not os.path.isfile(path):
        raise ValueError(f"{path}: the views have no {CAMERAS_FILE}")
    with open(path) as f:
        return sorted(json.load(f), key=lambda r: r["id"])


def _record_of(records: List[dict], path: str) -> dict:
    """the record at position int(stem), whose img_name must be the stem (View.load's assertion)"""
    stem = _stem(path)
    if int(stem) >= len(records) or records[int(stem)]["img_name"] != stem:
        found = records[int(stem)]["img_name"] if int(stem) < len(records) else None
        raise ValueError(f"{path}: the record at position {int(stem)} of {CAMERAS_FILE} is named {found!r}, not {stem!r}")
    return records[int(stem)]


def _positions(indices, count: int) -> List[int]:
    positions = list(range(count)) if indices is None else [int(i) for i in indices]
    for i in positions:
        if not 0 <= i < count:
            raise ValueError(f"{NAME}: indices: view {i} is not one of the {count} views")
    return positions


def read_cameras(directory: str) -> List[View]:
    """Every view of ``directory`` without its images (``near_far`` wants them all; they cost nothing)."""
    directory = os.fspath(directory)
    records = _records(directory)
    views = []
    for path in _listing(directory, NORMAL_DIRECTORY):
        record = _record_of(records, path)
        views.append(View(*camera_from_record(record), (record["height"], record["width"]), name=_stem(path)))
    return views


def read_views(directory: str, indices: Optional[Sequence[int]] = None, device="cuda", workers: int = 8,
               timings: Optional[Dict[str, float]] = None) -> List[View]:
    """``read_views(directory, mode=1)``: the views of ``directory`` sorted by the integer stem of their files, or those at
    the positions ``indices`` of that order, in the order of ``indices`` (no other file is opened).  ``ValueError``, naming
    the file, when a stem is not the ``img_name`` of its record, when ``cameras.json`` is missing, when the two images of a
    view differ in size, and for whatever ``decode_png_batch`` refuses.  ``timings``: a dict that receives the seconds of
    ``inflate``, ``upload``, ``unfilter`` and ``unpack`` (the GPU is then waited for after each)."""
    directory = os.fspath(directory)
    records = _records(directory)
    normals, colours = _listing(directory, NORMAL_DIRECTORY), _listing(directory, RGB_DIRECTORY)
    picked = _positions(indices, min(len(normals), len(colours)))           # the reference zips the two listings
    chosen = []
    for i in picked:
        if _stem(normals[i]) != _stem(colours[i]):
            raise ValueError(f"{normals[i]}: its colour image at the same position is {colours[i]}")
        chosen.append(_record_of(records, normals[i]))
    clock = _Clock(timings, torch.device(device))
    streams = _inflate_all([normals[i] for i in picked] + [colours[i] for i in picked], workers, device, clock)
    for k, i in enumerate(picked):                                          # before anything is uploaded
        (H, W, bpp), (Hc, Wc, _) = streams[k][0], streams[len(picked) + k][0]
        if (H, W) != (Hc, Wc):
            raise ValueError(f"{normals[i]}: {W} x {H}, but {colours[i]} is {Wc} x {Hc}")
        if bpp != 4:
            raise ValueError(f"{normals[i]}: a normal image carries the mask as its alpha; this one has no alpha")
    images = _unfilter_all(streams, device, clock)
    views = []
    for k, (i, record) in enumerate(zip(picked, chosen)):
        normal, mask, rgb = unpack_view(images[k], images[len(picked) + k])
        views.append(View(*camera_from_record(record), normal.shape[:2], normal, mask, rgb, name=_stem(normals[i])))
    clock.lap("unpack", gpu=True)
    return views


def read_fit_views(directory: str, indices: Optional[Sequence[int]] = None, device="cuda", workers: int = 8) -> list:
    """One ``texture_fit.FitView(c2w, K, rgb, mask)`` per image of ``gs_rendered_rgba/`` (stage 4's ``read_views``), or per
    position of ``indices``; the cameras are ``c2w_from_record``'s, float32."""
    from .texture_fit import FitView
    directory = os.fspath(directory)
    records = _records(directory)
    colours = _listing(directory, RGB_DIRECTORY)
    picked = _positions(indices, len(colours))
    chosen = [_record_of(records, colours[i]) for i in picked]
    clock = _Clock(None, torch.device(device))
    streams = _inflate_all([colours[i] for i in picked], workers, device, clock)
    for i, (geometry, _) in zip(picked, streams):
        if geometry[2] != 4:
            raise ValueError(f"{colours[i]}: a captured view carries the mask as its alpha; this one has no alpha")
    views = []
    for record, image in zip(chosen, _unfilter_all(streams, device, clock)):
        rgb, mask = unpack_rgba(image)
        c2w, K = c2w_from_record(record)
        views.append(FitView(c2w.astype(np.float32), K.astype(np.float32), rgb, mask))
    return views


# ---- the space --------------------------------------------------------------------------------------------------------

def _host(points) -> np.ndarray:
    return points.detach().cpu().numpy() if isinstance(points, torch.Tensor) else np.asarray(points)


class AABB:
    """The axis-aligned bounding box of ``points`` [N,3] (``deformer/utils/geometry.py``)."""

    def __init__(self, points):
        points = _host(points)
        self.min_p, self.max_p = np.amin(points, axis=0), np.amax(points, axis=0)

    @classmethod
    def load(cls, path):
        return cls(np.loadtxt(path).astype(np.float32))

    def save(self, path) -> None:
        np.savetxt(path, np.array(self.minmax))

    @property
    def minmax(self):
        return [self.min_p, self.max_p]

    @property
    def center(self):
        return 0.5 * (self.max_p + self.min_p)

    @property
    def longest_extent(self):
        return np.amax(self.max_p - self.min_p)

    @property
    def corners(self) -> np.ndarray:
        """[8,3]: the z = min face counter-clockwise from (min, min), then the z = max face likewise"""
        lo, hi = self.min_p, self.max_p
        xy = ((lo[0], lo[1]), (hi[0], lo[1]), (hi[0], hi[1]), (lo[0], hi[1]))
        return np.array([[x, y, z] for z in (lo[2], hi[2]) for x, y in xy])


def normalize_aabb(aabb: AABB, side_length: float = 1):
    """(``A``, ``A^-1``) float32 [4,4]: the scale and translation that take ``aabb`` into the cube of ``side_length`` about
    the origin, the longest extent filling it."""
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = -aabb.center
    s = side_length / aabb.longest_extent
    S = np.diag([s, s, s, 1]).astype(dtype=np.float32)
    A = S @ T
    return A, np.linalg.inv(A)


def _affine(points, M: np.ndarray):
    """``points @ M[:3,:3].T + M[:3,3]`` in float32: an array for an array, a tensor where it lives for a tensor"""
    if isinstance(points, torch.Tensor):
        m = torch.from_numpy(np.ascontiguousarray(M, dtype=np.float32)).to(points.device)
        return points.to(torch.float32) @ m[:3, :3].t() + m[:3, 3]
    return np.asarray(points) @ M[:3, :3].T + M[:3, 3][np.newaxis, :]


class SpaceNormalization:
    """The map ``A`` that takes the box of ``points`` into ``[-1, 1]^3`` and its application to views, vertices and boxes."""

    def __init__(self, points):
        self.aabb = AABB(points)
        self.A, self.A_inv = normalize_aabb(self.aabb, side_length=2)

    def normalize_views(self, views: Sequence[View]):
        for view in views:
            view.set_camera(*normalize_camera(*view.camera64, self.A))
        return views

    def normalize_mesh(self, vertices):
        return _affine(vertices, self.A)

    def normalize_aabb(self, aabb: AABB) -> AABB:
        return AABB(_affine(aabb.corners, self.A))

    def denormalize_mesh(self, vertices):
        return _affine(vertices, self.A_inv)


def near_far(views: Sequence[View], corners, epsilon: float = 0.5) -> Tuple[float, float]:
    """``Renderer.set_near_far``: with d the distances of ``corners`` [N,3] to the centres of ``views``,
    ``(min d - epsilon min d, max d + epsilon max d)``, in float32 on the host."""
    if len(views) == 0:
        raise ValueError(f"{NAME}: near_far needs at least one view")
    samples = torch.as_tensor(_host(corners), dtype=torch.float32)
    mins, maxs = [], []
    for view in views:
        d = view.project(samples, depth_as_distance=True)[..., 2]
        mins.append(d.min())
        maxs.append(d.max())
    near, far = min(mins), max(maxs)
    return float(near - near * epsilon), float(far + far * epsilon)


def view_mvps(views: Sequence[View], near: float, far: float) -> List[torch.Tensor]:
    """One ``GBufferRenderer.to_gl_camera`` matrix per view, as ``Deformer`` takes them"""
    return [GBufferRenderer.to_gl_camera(v.K, v.R, v.t, v.resolution, n=near, f=far) for v in views]


class ViewSampler:
    """``deformer/modules/view_sampler.py`` over POSITIONS: ``several`` keeps the views whose position in ``views`` is in
    ``picked_views``; a call draws ``views_per_iter`` positions of the kept list without replacement from numpy's global
    generator, the stream of the reference's draw over the list itself.  ``positions[k]`` is where kept view k sits in
    ``views``; ``__call__`` returns positions in ``views``."""
    modes = ["all", "several"]

    def __init__(self, views, mode: str = "all", views_per_iter: int = 1, picked_views=()):
        if mode not in self.modes:
            raise ValueError(f"Unknown mode '{mode}'. Available modes are {', '.join(self.modes)}")
        if mode == "several" and len(picked_views) == 0:
            raise ValueError("Empty picked_views when mode == several")
        self.mode, self.views_per_iter = mode, int(views_per_iter)
        picked = set(int(i) for i in picked_views)
        self.positions = [i for i in range(len(views)) if mode == "all" or i in picked]
        self.views = [views[i] for i in self.positions]

    def draw(self) -> np.ndarray:
        """positions in the KEPT list"""
        return np.random.choice(len(self.views), self.views_per_iter, replace=False)

    def __call__(self) -> List[int]:
        return [self.positions[int(k)] for k in self.draw()]


def adjust_template(vertices, bound: float) -> np.ndarray:
    """``adjust_and_scale_obj``: ``(x, y, z) -> (z, x, y) bound``, float64 in and out"""
    v = np.asarray(vertices, dtype=np.float64)
    return np.stack([v[:, 2], v[:, 0], v[:, 1]], axis=1) * bound
