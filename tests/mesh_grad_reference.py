"""torch-CPU statement of the CONTINUOUS functions whose derivatives the position gradients of the mesh render path are
(include/gd_mesh.h, "gradients to vertex positions"): the checker of tests/test_mesh_deform_*.py.  Parameterised by dtype:
float64 is the reference, float32 shows what the number format alone costs.  Gradients come from torch autograd.

The discrete decisions are not restated: they are taken from tests/mesh_reference.py (the triangle id per pixel from
``rasterize``; the chosen triangle, edge, side and branch of every antialias pair by the same walk as
``antialias_weights``, which tests/test_mesh_deform_cpu.py compares the result with).  Test infrastructure: never imported
by the package."""
import numpy as np
import torch

from tests import mesh_reference as ref


def big_triangle_scene(H=48, W=64):
    """(pos float32 [7,4], tri int32 [3,3]): three triangles whose shortest edge is well above 16 pixels at 64 x 48: two
    share an edge (a quad, with w different at every corner), the third lies nearer and covers a part of the second.
    Corners are given in pixels and carried to clip space."""
    px = np.array([[4.3, 5.2], [40.7, 9.1], [12.4, 40.3], [50.2, 38.6], [30.1, 20.3], [60.2, 14.8], [55.5, 44.9]])
    z = np.array([0.5, 0.5, 0.5, 0.5, 0.2, 0.2, 0.2])
    w = np.array([1.0, 1.5, 2.2, 1.2, 1.0, 1.3, 0.8])
    ndc = np.stack((2 * px[:, 0] / W - 1, 2 * px[:, 1] / H - 1, z), axis=1)
    pos = np.concatenate((ndc * w[:, None], w[:, None]), axis=1).astype(np.float32)
    return pos, np.array([[0, 1, 2], [2, 1, 3], [4, 5, 6]], dtype=np.int32)


def quad_scene(H, W, x0, x1, y0, y1, z=0.5):
    """(pos float32 [4,4], tri int32 [2,3]): the rectangle [x0, x1] x [y0, y1] (pixels; y grows with the row) as two
    triangles at w = 1."""
    px = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)
    pos = np.stack((2 * px[:, 0] / W - 1, 2 * px[:, 1] / H - 1, np.full(4, z), np.ones(4)), axis=1).astype(np.float32)
    return pos, np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def screen_xy(pos, H, W):
    """Unsnapped screen coordinates in pixels: sx = (x/w 0.5 + 0.5) W, sy = (y/w 0.5 + 0.5) H."""
    return (pos[:, 0] / pos[:, 3] * 0.5 + 0.5) * W, (pos[:, 1] / pos[:, 3] * 0.5 + 0.5) * H


def ideal_uv(pos, tri, ids):
    """(u, v) [H,W,2] of the header's continuous rasterize: pos torch [V,4], tri numpy [F,3], ids numpy int [H,W]
    (triangle + 1, 0 on background, where the result is 0)."""
    H, W = ids.shape
    flat = np.asarray(ids).ravel()
    hit = np.flatnonzero(flat > 0)
    t = torch.from_numpy(np.asarray(tri, dtype=np.int64)[flat[hit] - 1])
    fx = torch.from_numpy(2 * (hit % W) + 1).to(pos.dtype) / W - 1
    fy = torch.from_numpy(2 * (hit // W) + 1).to(pos.dtype) / H - 1
    P = pos[t]                                                  # [n, 3, 4]
    qx = P[..., 0] - fx[:, None] * P[..., 3]
    qy = P[..., 1] - fy[:, None] * P[..., 3]
    a0 = qx[:, 1] * qy[:, 2] - qy[:, 1] * qx[:, 2]
    a1 = qx[:, 2] * qy[:, 0] - qy[:, 2] * qx[:, 0]
    a2 = qx[:, 0] * qy[:, 1] - qy[:, 0] * qx[:, 1]
    S = (a0 + a1) + a2
    uv = torch.zeros(H * W, 2, dtype=pos.dtype)
    uv = uv.index_put((torch.from_numpy(hit),), torch.stack((a0 / S, a1 / S), dim=1))
    return uv.view(H, W, 2)


def forward_uv(pos, tri, rast):
    """The op as the package defines it: the VALUES of the snapped forward (``rast`` from mesh_reference.rasterize) with
    the DERIVATIVE of the continuous function."""
    ideal = ideal_uv(pos, tri, rast[..., 3].astype(np.int64))
    return torch.from_numpy(rast[..., :2].copy()).to(pos.dtype) + (ideal - ideal.detach())


def interpolate(attr, uv, ids, tri):
    """out [H,W,C] = u a0 + v a1 + (1 - u - v) a2, 0 on background."""
    t = torch.from_numpy(np.asarray(tri, dtype=np.int64)[np.maximum(np.asarray(ids) - 1, 0)])
    u, v = uv[..., 0:1], uv[..., 1:2]
    out = u * attr[t[..., 0]] + v * attr[t[..., 1]] + (1 - u - v) * attr[t[..., 2]]
    return out * torch.from_numpy(np.asarray(ids) > 0).to(attr.dtype)[..., None]


def antialias_pairs(rast, pos, tri, opp):
    """The decisions of the antialias analysis, by the header's rule, for every weight that is DEFINED (a pair that
    resolves to an edge with t <= 1), zero-valued ones included.  Dict of numpy arrays, one entry per weight:
    r, c, k (the element of wts [H,W,4] that receives it), a, b (the edge's vertices), horizontal, line, centre (of pixel
    I), sign (+1: w = t - 0.5 onto O, -1: w = 0.5 - t onto I), tri (the chosen triangle)."""
    H, W = rast.shape[:2]
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    tri = np.asarray(tri, dtype=np.int64)
    ok, X, Y, _, _ = ref.snap_vertices(pos, H, W)
    V = pos.shape[0]
    ids = rast[..., 3].astype(np.int64)
    zs = rast[..., 2]
    out = {k: [] for k in ("r", "c", "k", "a", "b", "horizontal", "line", "centre", "sign", "tri")}
    for r in range(H):
        for c in range(W):
            for k, (dr, dc) in enumerate(((0, -1), (0, 1), (-1, 0), (1, 0))):
                rn, cn = r + dr, c + dc
                if not (0 <= rn < H and 0 <= cn < W) or ids[r, c] == ids[rn, cn]:
                    continue
                idp, idn = ids[r, c], ids[rn, cn]
                if idp == 0:
                    inner = False
                elif idn == 0:
                    inner = True
                elif zs[r, c] != zs[rn, cn]:
                    inner = bool(zs[r, c] < zs[rn, cn])
                else:
                    inner = bool(idp < idn)
                t = int(idp if inner else idn) - 1
                ri, ci = (r, c) if inner else (rn, cn)
                horizontal = dr == 0
                vi = tri[t]
                if not ok[vi].all():
                    continue
                L = 256 * r + 128 if horizontal else 256 * c + 128
                line = np.float32(r if horizontal else c) + np.float32(0.5)
                centre = np.float32(ci if horizontal else ri) + np.float32(0.5)
                for i in range(3):
                    a, b, cc, d = int(vi[(i + 1) % 3]), int(vi[(i + 2) % 3]), int(vi[i]), int(opp[t, i])
                    if not (d < 0 or d >= V or not ok[d]):
                        ex, ey = int(X[b] - X[a]), int(Y[b] - Y[a])
                        sc = ex * int(Y[cc] - Y[a]) - ey * int(X[cc] - X[a])
                        sd = ex * int(Y[d] - Y[a]) - ey * int(X[d] - X[a])
                        if sc * sd < 0:
                            continue                                       # not a silhouette
                    a_on, b_on = (Y[a], Y[b]) if horizontal else (X[a], X[b])
                    a_al, b_al = (X[a], X[b]) if horizontal else (Y[a], Y[b])
                    if (a_on <= L) == (b_on <= L):
                        continue
                    f = np.float32
                    x = f(a_al) / f(256) + (f(b_al) / f(256) - f(a_al) / f(256)) * (
                        (line - f(a_on) / f(256)) / (f(b_on) / f(256) - f(a_on) / f(256)))
                    tt = np.abs(x - centre)
                    if not tt <= np.float32(1):
                        continue
                    outer = bool(tt > np.float32(0.5))
                    if outer != inner:                                     # this pixel is the one that receives
                        for key, val in zip(out, (r, c, k, a, b, horizontal, float(line), float(centre),
                                                  1.0 if outer else -1.0, t)):
                            out[key].append(val)
                    break
    return {k: np.asarray(v) for k, v in out.items()}


def ideal_weights(pos, pairs, H, W):
    """wts [H,W,4] of the header's continuous antialias analysis with the decisions ``pairs``: pos torch [V,4]."""
    # only the vertices of deciding edges are projected: an unusable vertex (w <= 0) elsewhere in the mesh has no screen
    # position and must not reach the graph
    sxa, sya = screen_xy(pos[torch.from_numpy(pairs["a"].astype(np.int64))], H, W)
    sxb, syb = screen_xy(pos[torch.from_numpy(pairs["b"].astype(np.int64))], H, W)
    hor = torch.from_numpy(pairs["horizontal"].astype(bool))
    al_a, al_b = torch.where(hor, sxa, sya), torch.where(hor, sxb, syb)
    on_a, on_b = torch.where(hor, sya, sxa), torch.where(hor, syb, sxb)
    line = torch.from_numpy(pairs["line"]).to(pos.dtype)
    centre = torch.from_numpy(pairs["centre"]).to(pos.dtype)
    x = al_a + (al_b - al_a) * ((line - on_a) / (on_b - on_a))
    w = torch.from_numpy(pairs["sign"]).to(pos.dtype) * (torch.abs(x - centre) - 0.5)
    index = tuple(torch.from_numpy(pairs[k].astype(np.int64)) for k in ("r", "c", "k"))
    return torch.zeros(H, W, 4, dtype=pos.dtype).index_put(index, w)


def forward_weights(pos, pairs, wts):
    """Values of the snapped analysis (``wts`` from mesh_reference.antialias_weights), derivative of the continuous one."""
    ideal = ideal_weights(pos, pairs, wts.shape[0], wts.shape[1])
    return torch.from_numpy(wts).to(pos.dtype) + (ideal - ideal.detach())


def antialias_apply(x, wts):
    """out = in + sum_k w_k (in[n_k] - in): mesh_reference.antialias_apply in differentiable torch."""
    z = torch.zeros_like(x)
    nbs = [torch.cat((z[:, :1], x[:, :-1]), 1), torch.cat((x[:, 1:], z[:, :1]), 1),
           torch.cat((z[:1], x[:-1]), 0), torch.cat((x[1:], z[:1]), 0)]
    acc = x
    for k, nb in enumerate(nbs):
        acc = acc + wts[..., k:k + 1] * (nb - x)
    return acc


# ---- the gradients the GPU tests compare with -------------------------------------------------------------------------

def _leaf(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).requires_grad_(True)


def grad_interpolate_rasterize(pos, tri, rast, attr, dout, dtype=torch.float64):
    """dL/dpos [V,4] (numpy float64) of L = sum(dout * interpolate(attr, rasterize(pos))), attr held fixed."""
    p = _leaf(pos, dtype)
    ids = rast[..., 3].astype(np.int64)
    out = interpolate(torch.from_numpy(attr).to(dtype), forward_uv(p, tri, rast), ids, tri)
    (out * torch.from_numpy(dout).to(dtype)).sum().backward()
    return p.grad.double().numpy()


def grad_antialias(pos, pairs, wts, color, dout, dtype=torch.float64):
    """dL/dpos [V,4] (numpy float64) of L = sum(dout * antialias(color; pos)), color held fixed."""
    p = _leaf(pos, dtype)
    out = antialias_apply(torch.from_numpy(color).to(dtype), forward_weights(p, pairs, wts))
    (out * torch.from_numpy(dout).to(dtype)).sum().backward()
    return p.grad.double().numpy()


def cancellation(pos, tri, rast, coeff, dtype=torch.float64):
    """(gradient through attr, gradient through rast), each [V,4] numpy float64, of
    L = sum_p coeff_p (P.x - fx P.w), P = interpolate(attr = pos).  For the continuous (u, v) the function is identically
    zero (sum_i a_i q_i = 0), so the two cancel; with the forward's snapped (u, v) the sum keeps the snapping term."""
    H, W = rast.shape[:2]
    ids = rast[..., 3].astype(np.int64)
    fx = (torch.arange(W, dtype=dtype) * 2 + 1) / W - 1
    c = torch.from_numpy(coeff).to(dtype)
    grads = []
    for through_attr in (True, False):
        p = _leaf(pos, dtype)
        attr = p if through_attr else p.detach()
        uv = forward_uv(p, tri, rast)
        P = interpolate(attr, uv if not through_attr else uv.detach(), ids, tri)
        (c * (P[..., 0] - fx[None, :] * P[..., 3])).sum().backward()
        grads.append(p.grad.double().numpy())
    return grads[0], grads[1]


def normalised_error(g, g64):
    """max |g - g64| / max |g64|"""
    return float(np.abs(np.asarray(g, dtype=np.float64) - g64).max() / np.abs(g64).max())
