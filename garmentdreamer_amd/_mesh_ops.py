"""The mesh render ops themselves, once: per-mesh topology (host, numpy) and the three autograd functions over the HIP
kernels of ``csrc/raster_mesh.hip`` (include/gd_mesh.h, include/gd_mesh_deform.h).  ``mesh_render`` (fixed geometry) and
``mesh_deform`` (moving geometry) are the two policies over them: they validate, decide what is detached, and call these.
Every backward produces exactly the gradients ``ctx.needs_input_grad`` asks for, so an input that was detached costs
nothing.  All tensors here are contiguous and without a minibatch axis; that is the callers' business."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _native
from ._launch import launch, scratch


class MeshTopology(NamedTuple):
    opp: torch.Tensor          # int32 [F,3]: vertex across edge i (opposite vertex i), -1 unless exactly 2 triangles share it
    corner_ptr: torch.Tensor   # int32 [V+1]
    corner_idx: torch.Tensor   # int32 [3F]: corners 3 t + i of each vertex, ascending


def _unbatch(name: str, what: str, t: torch.Tensor, dims: int):
    """(tensor without the minibatch axis, had one)"""
    if t.dim() == dims + 1:
        if t.shape[0] != 1:
            raise ValueError(f"{name}: {what} has a minibatch of {t.shape[0]}; one image per call")
        return t[0], True
    if t.dim() != dims:
        raise ValueError(f"{name}: {what} must have {dims} dimensions (or {dims + 1} with a minibatch of 1)")
    return t, False


def host_triangles(tri, num_vertices: Optional[int], device):
    """(int64 [F,3] numpy, V, device) of ``tri`` (tensor or array [F,3]); the device defaults to that of a tensor"""
    if isinstance(tri, torch.Tensor):
        device = tri.device if device is None else device
        t = tri.detach().cpu().numpy()
    else:
        t = np.asarray(tri)
    t = np.ascontiguousarray(t, dtype=np.int64).reshape(-1, 3)
    nv = int(num_vertices) if num_vertices is not None else (int(t.max()) + 1 if t.shape[0] else 0)
    return t, nv, device


def edge_groups(t: np.ndarray, nv: int):
    """The 3F edges of ``t`` grouped by their vertex pair.  Edge i of triangle f runs between corners i+1 and i+2 and is
    k = 3 f + i.  Returns (lo, hi, order, start, count): the smaller and larger vertex of each k, the stable order that
    sorts the k by (lo, hi), and of each distinct pair the position of its first k in that order and how many share it."""
    lo = np.minimum(t[:, [1, 2, 0]], t[:, [2, 0, 1]]).ravel()
    hi = np.maximum(t[:, [1, 2, 0]], t[:, [2, 0, 1]]).ravel()
    key = lo * max(nv, 1) + hi
    order = np.argsort(key, kind="stable")
    sk = key[order]
    start = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]]) if t.shape[0] else np.zeros(0, np.int64)
    return lo, hi, order, start, np.diff(np.r_[start, sk.shape[0]])


def build_topology(tri, num_vertices: Optional[int] = None, device=None) -> MeshTopology:
    """Per-mesh topology of ``tri`` (tensor or array [F,3]), computed on the host with numpy and uploaded to ``device``
    (default: the device of ``tri`` if it is a tensor, else the CPU)."""
    t, nv, device = host_triangles(tri, num_vertices, device)
    nf = t.shape[0]
    if nf and (t.min() < 0 or t.max() >= nv):
        raise ValueError("build_topology: vertex index out of range")
    _, _, order, start, count = edge_groups(t, nv)
    first = start[count == 2]
    a, b = order[first], order[first + 1]
    opp = np.full(3 * nf, -1, dtype=np.int32)
    own = t.ravel()                                     # an edge's own opposite vertex is corner i
    opp[a], opp[b] = own[b], own[a]
    corners = np.argsort(own, kind="stable")
    ptr = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(np.bincount(own, minlength=nv), out=ptr[1:])
    dev = torch.device("cpu") if device is None else torch.device(device)
    return MeshTopology(torch.from_numpy(opp.reshape(nf, 3)).to(dev), torch.from_numpy(ptr.astype(np.int32)).to(dev),
                        torch.from_numpy(corners.astype(np.int32)).to(dev))


def rasterize_forward(pos: torch.Tensor, tri: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """``rast`` [H,W,4] of ``pos`` [V,4] / ``tri`` [F,3], outside autograd: what both modules call for fixed positions"""
    nf = tri.shape[0]
    rast = torch.empty((H, W, 4), dtype=torch.float32, device=pos.device)
    launch("gd_mesh_rasterize", pos.device, pos.shape[0], nf, H, W, pos, tri, rast,
           scratch(_native.lib().gd_mesh_rasterize_scratch_bytes(nf, H, W), pos.device))
    return rast


class _Rasterize(torch.autograd.Function):
    """``rasterize_forward`` with the gradient to ``pos``, which needs ``topology``"""

    @staticmethod
    def forward(ctx, pos, tri, H, W, topology):
        rast = rasterize_forward(pos, tri, H, W)
        ctx.save_for_backward(pos, tri, rast)
        ctx.topology = topology
        return rast

    @staticmethod
    def backward(ctx, drast):
        pos, tri, rast = ctx.saved_tensors
        dev = pos.device
        H, W = rast.shape[:2]
        V, nf = pos.shape[0], tri.shape[0]
        dpos = torch.empty((V, 4), dtype=torch.float32, device=dev)
        launch("gd_mesh_rasterize_backward", dev, V, nf, H, W, pos, tri, rast, drast.contiguous(),
               ctx.topology.corner_ptr, ctx.topology.corner_idx, dpos,
               scratch(_native.lib().gd_mesh_rasterize_backward_scratch_bytes(nf), dev))
        return dpos, None, None, None, None


class _Interpolate(torch.autograd.Function):
    """``out`` [H,W,C] of ``attr`` [V,C]; gradients to ``attr`` (needs ``pos``, what ``rast`` was made from, and
    ``topology``) and to ``rast``.  ``pos=None``: forward only."""

    @staticmethod
    def forward(ctx, attr, rast, tri, pos, topology):
        dev = attr.device
        H, W = rast.shape[:2]
        V, C = attr.shape
        out = torch.empty((H, W, C), dtype=torch.float32, device=dev)
        launch("gd_mesh_interpolate_forward", dev, V, tri.shape[0], C, H, W, attr, rast, tri, out)
        ctx.save_for_backward(attr, rast, tri, pos)
        ctx.topology = topology
        return out

    @staticmethod
    def backward(ctx, dout):
        attr, rast, tri, pos = ctx.saved_tensors
        dev = rast.device
        H, W = rast.shape[:2]
        V, C = attr.shape
        nf = tri.shape[0]
        dout = dout.contiguous()
        dattr = drast = None
        if ctx.needs_input_grad[0]:
            if ctx.topology is None or pos is None:
                raise RuntimeError("interpolate: the gradient to attr needs pos= (the positions rast came from)")
            dattr = torch.empty((V, C), dtype=torch.float32, device=dev)
            launch("gd_mesh_interpolate_backward", dev, V, nf, C, H, W, pos, tri, rast, dout, ctx.topology.corner_ptr,
                   ctx.topology.corner_idx, dattr,
                   scratch(_native.lib().gd_mesh_interpolate_backward_scratch_bytes(nf, C), dev))
        if ctx.needs_input_grad[1]:
            drast = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
            launch("gd_mesh_interpolate_backward_rast", dev, V, nf, C, H, W, attr, rast, tri, dout, drast)
        return dattr, drast, None, None, None


def aa_apply(x: torch.Tensor, wts: torch.Tensor, adjoint: bool) -> torch.Tensor:
    H, W, C = x.shape
    out = torch.empty_like(x)
    launch("gd_mesh_antialias_apply", x.device, C, H, W, x, wts, out, int(adjoint))
    return out


class _Antialias(torch.autograd.Function):
    """The blend of ``color`` [H,W,C] by the analysis ``wts``; gradients to ``color`` (the adjoint blend) and to ``pos``
    (needs ``rast``, ``tri`` and ``topology``).  ``pos=None``: fixed geometry, nothing but ``wts`` is kept."""

    @staticmethod
    def forward(ctx, color, wts, pos, rast, tri, topology):
        if pos is None:
            ctx.save_for_backward(wts)
        else:
            ctx.save_for_backward(wts, color, pos, rast, tri)
        ctx.topology = topology
        return aa_apply(color, wts, False)

    @staticmethod
    def backward(ctx, dout):
        wts, *moving = ctx.saved_tensors
        dout = dout.contiguous()
        dcolor = aa_apply(dout, wts, True) if ctx.needs_input_grad[0] else None
        dpos = None
        if ctx.needs_input_grad[2]:
            color, pos, rast, tri = moving
            dev = pos.device
            H, W, C = color.shape
            V, nf = pos.shape[0], tri.shape[0]
            topo = ctx.topology
            dpos = torch.empty((V, 4), dtype=torch.float32, device=dev)
            launch("gd_mesh_antialias_backward_pos", dev, V, nf, C, H, W, rast, pos, tri, topo.opp, color, dout,
                   topo.corner_ptr, topo.corner_idx, dpos,
                   scratch(_native.lib().gd_mesh_antialias_backward_pos_scratch_bytes(nf), dev))
        return dcolor, None, dpos, None, None, None
