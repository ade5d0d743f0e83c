"""Mesh render path of the NeTF stage: the three nvdiffrast operations ``Renderer.render`` rests on
(Garment_Deformer_NeTF/netf/render/mesh_renderer.py:338-428), on the HIP kernels of ``csrc/raster_mesh.hip``
(C-ABI and definitions: include/gd_mesh.h) -- no CPU path.

  * ``rasterize(pos, tri, resolution)``                    <- ``dr.rasterize``   (no GL context; returns ``rast`` only)
  * ``interpolate(attr, rast, tri)``                        <- ``dr.interpolate`` (gradient to ``attr``)
  * ``antialias(color, rast, pos, tri, topology, weights)`` <- ``dr.antialias``   (gradient to ``color``)
  * ``build_topology(tri)``   per-mesh host work (numpy): opposite vertices for the silhouette test and the CSR list
                              of each vertex's corners for the atomics-free attribute gradient
  * ``MeshRenderer``          ``Renderer.render`` for ``fix_geo: true`` / ``ssaa = 1``
  * ``projection`` / ``perspective``  the reference's camera matrices (numpy)

Two limits, both outside the reference's live configuration: there is no gradient with respect to vertex positions in
this module (``pos.requires_grad`` raises; moving geometry is ``mesh_deform``), and no near-plane clipping (a triangle with
a vertex at ``w <= 0`` is dropped).
Tensors follow nvdiffrast's shapes with the minibatch axis optional: ``pos`` [V,4] or [1,V,4], ``rast`` [H,W,4] or
[1,H,W,4], and so on; the output has a batch axis iff the image input had one.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import _native

MAX_CHANNELS = 8
_POS_GRAD = ("gradients with respect to vertex positions are not implemented (nvdiffrast's rast_db and the position "
             "gradient of antialias): detach pos, or keep the geometry fixed (fix_geo: true)")


class MeshTopology(NamedTuple):
    opp: torch.Tensor          # int32 [F,3]: vertex across edge i (opposite vertex i), -1 unless exactly 2 triangles share it
    corner_ptr: torch.Tensor   # int32 [V+1]
    corner_idx: torch.Tensor   # int32 [3F]: corners 3 t + i of each vertex, ascending


def _check(ret: int, what: str) -> None:
    if ret < 0:
        raise RuntimeError(f"{what} failed ({ret}): {_native.lib().gd_mesh_last_error().decode('utf-8', 'replace')}")


def _gpu(name: str, what: str, t: torch.Tensor, dtype, last: Optional[int]) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: the HIP kernels have no CPU path ({what} must be on the GPU)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: {what} must be {dtype}")
    if last is not None and (t.dim() < 2 or t.shape[-1] != last):
        raise ValueError(f"{name}: {what} must be [..., {last}]")
    return t


def _unbatch(name: str, what: str, t: torch.Tensor, dims: int):
    """(tensor without the minibatch axis, had one)"""
    if t.dim() == dims + 1:
        if t.shape[0] != 1:
            raise ValueError(f"{name}: {what} has a minibatch of {t.shape[0]}; one image per call")
        return t[0], True
    if t.dim() != dims:
        raise ValueError(f"{name}: {what} must have {dims} dimensions (or {dims + 1} with a minibatch of 1)")
    return t, False


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def build_topology(tri, num_vertices: Optional[int] = None, device=None) -> MeshTopology:
    """Per-mesh topology of ``tri`` (tensor or array [F,3]), computed on the host with numpy and uploaded to ``device``
    (default: the device of ``tri`` if it is a tensor, else the CPU)."""
    if isinstance(tri, torch.Tensor):
        device = tri.device if device is None else device
        t = tri.detach().cpu().numpy()
    else:
        t = np.asarray(tri)
    t = np.ascontiguousarray(t, dtype=np.int64).reshape(-1, 3)
    nf = t.shape[0]
    nv = int(num_vertices) if num_vertices is not None else (int(t.max()) + 1 if nf else 0)
    if nf and (t.min() < 0 or t.max() >= nv):
        raise ValueError("build_topology: vertex index out of range")
    # edge i of triangle t runs between vertices i+1 and i+2; its own opposite vertex is i
    lo = np.minimum(t[:, [1, 2, 0]], t[:, [2, 0, 1]]).ravel()
    hi = np.maximum(t[:, [1, 2, 0]], t[:, [2, 0, 1]]).ravel()
    key = lo * max(nv, 1) + hi
    order = np.argsort(key, kind="stable")
    sk = key[order]
    start = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]]) if nf else np.zeros(0, np.int64)
    count = np.diff(np.r_[start, sk.shape[0]])
    first = start[count == 2]
    a, b = order[first], order[first + 1]
    opp = np.full(3 * nf, -1, dtype=np.int32)
    own = t.ravel()
    opp[a], opp[b] = own[b], own[a]
    corners = np.argsort(own, kind="stable")
    ptr = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(np.bincount(own, minlength=nv), out=ptr[1:])
    dev = torch.device("cpu") if device is None else torch.device(device)
    return MeshTopology(torch.from_numpy(opp.reshape(nf, 3)).to(dev), torch.from_numpy(ptr.astype(np.int32)).to(dev),
                        torch.from_numpy(corners.astype(np.int32)).to(dev))


def rasterize(pos: torch.Tensor, tri: torch.Tensor, resolution) -> torch.Tensor:
    """``rast`` float32 [H,W,4] = (u, v, z/w, triangle id + 1), zeros where nothing is covered ([1,H,W,4] if ``pos`` is
    [1,V,4]).  ``pos``: float32 clip-space positions [V,4]; ``tri``: int32 [F,3]; ``resolution``: (H, W).  Row 0 is
    ``y_ndc = -1``.  Not differentiable."""
    _gpu("rasterize", "pos", pos, torch.float32, 4)
    _gpu("rasterize", "tri", tri, torch.int32, 3)
    if pos.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("rasterize: " + _POS_GRAD)
    p, batched = _unbatch("rasterize", "pos", pos.detach(), 2)
    H, W = int(resolution[0]), int(resolution[1])
    p, t = p.contiguous(), tri.contiguous()
    if t.dim() != 2:
        raise ValueError("rasterize: tri must be [F,3]")
    dev = p.device
    L = _native.lib()
    V, nf = p.shape[0], t.shape[0]
    rast = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    scratch = torch.empty(max(L.gd_mesh_rasterize_scratch_bytes(nf, H, W), 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(L.gd_mesh_rasterize(_stream(dev), V, nf, H, W, p.data_ptr(), t.data_ptr(), rast.data_ptr(),
                                   scratch.data_ptr()), "gd_mesh_rasterize")
    return rast[None] if batched else rast


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, tri, pos, topology):
        dev = attr.device
        H, W = rast.shape[:2]
        V, C = attr.shape
        out = torch.empty((H, W, C), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _check(_native.lib().gd_mesh_interpolate_forward(_stream(dev), V, tri.shape[0], C, H, W, attr.data_ptr(),
                                                             rast.data_ptr(), tri.data_ptr(), out.data_ptr()),
                   "gd_mesh_interpolate_forward")
        ctx.save_for_backward(rast, tri, pos if pos is not None else attr.new_empty(0))
        ctx.topology, ctx.shape = topology, (V, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        rast, tri, pos = ctx.saved_tensors
        if ctx.topology is None or pos.numel() == 0:
            raise RuntimeError("interpolate: the gradient to attr needs pos= (the positions rast came from)")
        V, C = ctx.shape
        dev = rast.device
        H, W = rast.shape[:2]
        nf = tri.shape[0]
        L = _native.lib()
        dout = dout.contiguous()
        dattr = torch.empty((V, C), dtype=torch.float32, device=dev)
        scratch = torch.empty(max(L.gd_mesh_interpolate_backward_scratch_bytes(nf, C), 1), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _check(L.gd_mesh_interpolate_backward(_stream(dev), V, nf, C, H, W, pos.data_ptr(), tri.data_ptr(),
                                                  rast.data_ptr(), dout.data_ptr(), ctx.topology.corner_ptr.data_ptr(),
                                                  ctx.topology.corner_idx.data_ptr(), dattr.data_ptr(),
                                                  scratch.data_ptr()), "gd_mesh_interpolate_backward")
        return dattr, None, None, None, None


def interpolate(attr: torch.Tensor, rast: torch.Tensor, tri: torch.Tensor, pos: Optional[torch.Tensor] = None,
                topology: Optional[MeshTopology] = None) -> torch.Tensor:
    """``out`` [H,W,C] = (u a0 + v a1) + (1 - u - v) a2 of the covering triangle's corner attributes, 0 on background.
    ``attr``: float32 [V,C], C <= 8.  The gradient to ``attr`` walks each triangle's pixel box again and sums each
    vertex's corners in a fixed order (no atomics, bit-reproducible): it needs ``pos`` (what ``rast`` was made from) and
    uses ``topology`` (``build_topology(tri)`` if missing: a host pass over the mesh).  Without ``pos`` the op is
    forward-only and raises if ``attr`` requires a gradient."""
    _gpu("interpolate", "attr", attr, torch.float32, None)
    _gpu("interpolate", "rast", rast, torch.float32, 4)
    _gpu("interpolate", "tri", tri, torch.int32, 3)
    a, b1 = _unbatch("interpolate", "attr", attr, 2)
    r, b2 = _unbatch("interpolate", "rast", rast.detach(), 3)
    if not 1 <= a.shape[1] <= MAX_CHANNELS:
        raise ValueError(f"interpolate: attr must have 1..{MAX_CHANNELS} channels")
    p = None
    if pos is not None:
        _gpu("interpolate", "pos", pos, torch.float32, 4)
        if pos.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("interpolate: " + _POS_GRAD)
        p = _unbatch("interpolate", "pos", pos.detach(), 2)[0].contiguous()
        if p.shape[0] != a.shape[0]:
            raise ValueError("interpolate: pos and attr must have one row per vertex")
    if a.requires_grad and torch.is_grad_enabled():
        if p is None:
            raise RuntimeError("interpolate: the gradient to attr walks each triangle's pixel box again and needs pos= "
                               "(the clip-space positions rast was made from)")
        if topology is None:
            topology = build_topology(tri, num_vertices=a.shape[0], device=a.device)
    if topology is not None:
        if not topology.corner_ptr.is_cuda or topology.corner_ptr.shape[0] != a.shape[0] + 1 \
                or topology.corner_idx.shape[0] != 3 * tri.shape[0]:
            raise ValueError("interpolate: topology does not belong to this mesh (or is not on the GPU)")
    out = _Interpolate.apply(a.contiguous(), r.contiguous(), tri.contiguous(), p, topology)
    return out[None] if (b1 or b2) else out


def antialias_weights(rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor, topology: MeshTopology) -> torch.Tensor:
    """``wts`` float32 [H,W,4]: the silhouette analysis of (rast, pos), shared by every image antialiased with them."""
    _gpu("antialias", "rast", rast, torch.float32, 4)
    _gpu("antialias", "pos", pos, torch.float32, 4)
    _gpu("antialias", "tri", tri, torch.int32, 3)
    if pos.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("antialias: " + _POS_GRAD)
    r = _unbatch("antialias", "rast", rast.detach(), 3)[0].contiguous()
    p = _unbatch("antialias", "pos", pos.detach(), 2)[0].contiguous()
    t = tri.contiguous()
    if not topology.opp.is_cuda or tuple(topology.opp.shape) != tuple(t.shape):
        raise ValueError("antialias: topology does not belong to this mesh (or is not on the GPU)")
    dev = r.device
    H, W = r.shape[:2]
    wts = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _check(_native.lib().gd_mesh_antialias_weights(_stream(dev), p.shape[0], t.shape[0], H, W, r.data_ptr(),
                                                       p.data_ptr(), t.data_ptr(), topology.opp.contiguous().data_ptr(),
                                                       wts.data_ptr()), "gd_mesh_antialias_weights")
    return wts


def _aa_apply(x: torch.Tensor, wts: torch.Tensor, adjoint: bool) -> torch.Tensor:
    dev = x.device
    H, W, C = x.shape
    out = torch.empty_like(x)
    with torch.cuda.device(dev):
        _check(_native.lib().gd_mesh_antialias_apply(_stream(dev), C, H, W, x.data_ptr(), wts.data_ptr(), out.data_ptr(),
                                                     int(adjoint)), "gd_mesh_antialias_apply")
    return out


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, wts):
        ctx.save_for_backward(wts)
        return _aa_apply(color, wts, False)

    @staticmethod
    def backward(ctx, dout):
        (wts,) = ctx.saved_tensors
        return _aa_apply(dout.contiguous(), wts, True), None


def antialias(color: torch.Tensor, rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor,
              topology: Optional[MeshTopology] = None, weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dr.antialias``: blends ``color`` [H,W,C] across silhouette edges.  The analysis depends on (rast, pos) only:
    pass ``weights=antialias_weights(...)`` to share it between images (``topology`` is then not needed); otherwise it
    is computed here from ``topology`` (``build_topology(tri)`` if that is missing too: a host pass over the mesh)."""
    _gpu("antialias", "color", color, torch.float32, None)
    c, batched = _unbatch("antialias", "color", color, 3)
    if weights is None:
        if topology is None:
            topology = build_topology(tri, num_vertices=pos.shape[-2], device=color.device)
        weights = antialias_weights(rast, pos, tri, topology)
    else:
        _gpu("antialias", "weights", weights, torch.float32, 4)
        if pos is not None and isinstance(pos, torch.Tensor) and pos.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("antialias: " + _POS_GRAD)
    if tuple(weights.shape) != (c.shape[0], c.shape[1], 4):
        raise ValueError("antialias: weights must be [H,W,4] of the colour's resolution")
    out = _Antialias.apply(c.contiguous(), weights.contiguous())
    return out[None] if batched else out


def projection(fx, fy, cx, cy, width, height, n=0.01, f=1000):
    """``Renderer.projection`` (mesh_renderer.py:242-246): OpenGL projection from pinhole intrinsics, float32 [4,4]."""
    return np.array([[2.0 * fx / width, 0, 1.0 - 2.0 * cx / width, 0],
                     [0, 2.0 * fy / height, 1.0 - 2.0 * cy / height, 0],
                     [0, 0, -(f + n) / (f - n), -(2 * f * n) / (f - n)],
                     [0, 0, -1, 0.0]], dtype=np.float32)


def perspective(fovy, near=0.01, far=100):
    """``netf/view_core/camera.py:4-26``: ``fovy`` in radians, aspect 1, y flipped; float32 [4,4]."""
    y = np.tan(fovy / 2)
    return np.array([[1 / y, 0, 0, 0],
                     [0, -1 / y, 0, 0],
                     [0, 0, -(far + near) / (far - near), -(2 * far * near) / (far - near)],
                     [0, 0, -1, 0]], dtype=np.float32)


def safe_normalize(x: torch.Tensor, eps: float = 1e-20) -> torch.Tensor:
    """kiui.op.safe_normalize"""
    return x / torch.sqrt(torch.clamp(torch.sum(x * x, -1, keepdim=True), min=eps))


class MeshRenderer:
    """``Renderer.render`` (mesh_renderer.py:338-428) for ``fix_geo: true``: a fixed mesh ``v`` [V,3] / ``f`` [F,3] with
    vertex normals ``vn`` [V,3], coloured by ``texture_fn``: any callable [N,3] -> [N,3] in [0,1] evaluated at the
    visible surface points (the reference's ``sigmoid(mlp(encoder(xyz)))``)."""

    def __init__(self, v: torch.Tensor, f: torch.Tensor, vn: torch.Tensor, texture_fn: Callable):
        _gpu("MeshRenderer", "v", v, torch.float32, 3)
        _gpu("MeshRenderer", "vn", vn, torch.float32, 3)
        if not isinstance(f, torch.Tensor) or not f.is_cuda:
            raise RuntimeError("MeshRenderer: the HIP kernels have no CPU path (f must be on the GPU)")
        if v.requires_grad or vn.requires_grad:
            raise NotImplementedError("MeshRenderer: " + _POS_GRAD)
        self.v = v.detach().contiguous()
        self.f = f.detach().to(torch.int32).contiguous()
        self.vn = vn.detach().contiguous()
        self.texture_fn = texture_fn
        self.topology = build_topology(self.f, num_vertices=self.v.shape[0], device=self.v.device)

    def clip_positions(self, pose, proj):
        """(v_cam [V,4], v_clip [V,4]) of the mesh under ``pose`` / ``proj`` (numpy [4,4]), as ``render`` forms them."""
        v = self.v
        pose = torch.from_numpy(np.asarray(pose).astype(np.float32)).to(v.device)
        proj = torch.from_numpy(np.asarray(proj).astype(np.float32)).to(v.device)
        v_cam = torch.matmul(F.pad(v, pad=(0, 1), mode="constant", value=1.0), torch.inverse(pose).T).float()
        return v_cam, (v_cam @ proj.T).contiguous()

    def render(self, pose, proj, h0, w0, ssaa=1, bg_color=1):
        """``pose`` (camera to world) and ``proj``: numpy [4,4].  Returns the reference's dict: ``image`` [H,W,3],
        ``alpha`` [H,W,1], ``depth`` [H,W,1], ``normal`` [H,W,3] in [0,1], ``cosinesview`` [H,W]."""
        if ssaa != 1:
            raise ValueError("MeshRenderer.render: ssaa != 1 is not implemented (the reference's trainer passes 1)")
        h, w = int(h0), int(w0)
        v, f, topo = self.v, self.f, self.topology
        v_cam, v_clip = self.clip_positions(pose, proj)
        pose = torch.from_numpy(np.asarray(pose).astype(np.float32)).to(v.device)

        rast = rasterize(v_clip, f, (h, w))
        wts = antialias_weights(rast, v_clip, f, topo)      # one analysis for alpha, colour, position and normal

        alpha = torch.clamp(rast[..., -1:], 0, 1).contiguous()
        alpha = antialias(alpha, rast, v_clip, f, weights=wts).clamp(0, 1)
        depth = interpolate(-v_cam[..., [2]].contiguous(), rast, f)
        xyzs_ = interpolate(v, rast, f)
        xyzs = xyzs_.view(-1, 3)
        mask = (alpha > 0).view(-1)
        color = torch.zeros_like(xyzs, dtype=torch.float32)
        if mask.any():
            color[mask] = self.texture_fn(xyzs[mask]).float()
        color = color.view(h, w, 3)
        color = antialias(color, rast, v_clip, f, weights=wts).clamp(0, 1)
        color = alpha * color + (1 - alpha) * bg_color

        normal_ = interpolate(self.vn, rast, f)
        normal = safe_normalize(normal_)
        with torch.no_grad():
            position = antialias(xyzs_, rast, v_clip, f, weights=wts)
            normal_aa = antialias(normal_, rast, v_clip, f, weights=wts)
            view_direction = F.normalize(position - pose[:3, 3], dim=-1)
            cosines_view = F.cosine_similarity(view_direction, normal_aa, dim=-1, eps=1e-6)
        return {"image": color, "alpha": alpha, "depth": depth, "normal": (normal + 1) / 2, "cosinesview": cosines_view}
