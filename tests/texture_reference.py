"""The definitions of include/gd_texture.h in numpy and torch on the CPU, by dtype: the REFERENCE of the texture-field tests.

  * ``layout(...)``                      the level table (float64 numpy), stated here independently of the package
  * ``encode(x, grid, lay, mask)``       the encoding, vectorised; differentiable with respect to ``grid`` (autograd)
  * ``encode_level_looped(...)``         one level of it again with plain Python loops over points and corners
  * ``encode_backward(...)``             ``dgrid`` by ``index_add_``
  * ``field(...)`` / ``field_backward(...)``  the fused field and its gradients from the formulas of the header;
    ``order`` permutes the points first, which changes nothing but the order of every sum over points, and
    ``sequential=True`` adds the MLP gradients one point after the other instead of through torch's matrix product

In float32 every operation of the encoding is one IEEE operation in the order the header writes (torch's CPU kernels do not
fuse a multiply into an add), so ``encode`` in float32 is what the GPU must return bit for bit.  The integer arithmetic
is numpy uint32, which wraps."""
import math

import numpy as np
import torch

PRIME1, PRIME2 = np.uint32(2654435761), np.uint32(805459861)
FEATURES = 2


def layout(num_levels=16, base_resolution=16, per_level_scale=None, log2_hashmap_size=19):
    """dict: scale float32 [L], res / size int64 [L], offset int64 [L + 1], dense bool [L]"""
    if per_level_scale is None:
        per_level_scale = 2.0 ** (math.log2(1024 / 16) / 15)
    scale, res, size = [], [], []
    for l in range(num_levels):
        s = np.float32(2.0 ** (l * math.log2(per_level_scale)) * base_resolution - 1.0)
        r = int(math.ceil(float(s))) + 1
        scale.append(s)
        res.append(r)
        size.append(min((r ** 3 + 7) // 8 * 8, 2 ** log2_hashmap_size))
    res, size = np.array(res, dtype=np.int64), np.array(size, dtype=np.int64)
    return dict(num_levels=num_levels, scale=np.array(scale, dtype=np.float32), res=res, size=size,
                offset=np.concatenate(([0], np.cumsum(size))).astype(np.int64), dense=res ** 3 <= size)


def valid_rows(x, mask=None):
    ok = torch.isfinite(x).all(dim=1)
    if mask is not None:
        ok = ok & (mask != 0)
    return ok


def _cells(u, lay, l):
    """per corner i: (index into the level int64 [N], weight [N]) for unit-cube coordinates ``u`` [N,3]"""
    p = u * float(lay["scale"][l])
    p = p + 0.5
    fl = torch.floor(p)
    w = p - fl
    c = fl.to(torch.int32).numpy().view(np.uint32)                     # (uint32)(int32)floor
    res, size = np.uint32(lay["res"][l]), np.uint32(lay["size"][l])
    out = []
    with np.errstate(over="ignore"):
        for i in range(8):
            d = [np.uint32((i >> k) & 1) for k in range(3)]
            g = [c[:, k] + d[k] for k in range(3)]
            if lay["dense"][l]:
                idx = g[0] + g[1] * res + g[2] * res * res
            else:
                idx = g[0] ^ (g[1] * PRIME1) ^ (g[2] * PRIME2)
            idx = idx % size
            wt = [w[:, k] if d[k] else 1 - w[:, k] for k in range(3)]
            out.append((torch.from_numpy(idx.astype(np.int64)), (wt[0] * wt[1]) * wt[2]))
    return out


def _unit(x, grid_dtype, mask):
    x = x.detach().to(grid_dtype)
    ok = valid_rows(x, mask)
    xs = torch.where(ok[:, None], x, torch.zeros_like(x))             # a finite stand-in; its output is zeroed below
    return (xs + 1) * 0.5, ok


def encode(x, grid, lay, mask=None):
    """[N, L F] of ``grid``'s dtype"""
    u, ok = _unit(x, grid.dtype, mask)
    table = grid.view(-1, FEATURES)
    cols = []
    for l in range(lay["num_levels"]):
        acc = torch.zeros(x.shape[0], FEATURES, dtype=grid.dtype)
        for idx, wt in _cells(u, lay, l):
            acc = acc + wt[:, None] * table[int(lay["offset"][l]) + idx]
        cols.append(acc)
    enc = torch.cat(cols, dim=1)
    return torch.where(ok[:, None], enc, torch.zeros_like(enc))


def encode_level_looped(x, grid, lay, l, mask=None):
    """[N, F]: level ``l`` of ``encode`` with Python scalars of numpy's types, one point and one corner at a time"""
    ft = {torch.float32: np.float32, torch.float64: np.float64}[grid.dtype]
    g = grid.detach().numpy().reshape(-1, FEATURES)
    xs = x.detach().numpy().astype(ft)
    out = np.zeros((xs.shape[0], FEATURES), dtype=ft)
    s, res, size, off = ft(lay["scale"][l]), int(lay["res"][l]), int(lay["size"][l]), int(lay["offset"][l])
    for n in range(xs.shape[0]):
        if not np.isfinite(xs[n]).all() or (mask is not None and not mask[n]):
            continue
        c, w = [], []
        for k in range(3):
            p = s * ((xs[n, k] + ft(1)) * ft(0.5))
            p = p + ft(0.5)
            fl = np.floor(p)
            c.append(int(fl) % 2 ** 32)
            w.append(p - fl)
        for i in range(8):
            d = [(i >> k) & 1 for k in range(3)]
            gc = [(c[k] + d[k]) % 2 ** 32 for k in range(3)]
            if lay["dense"][l]:
                idx = (gc[0] + gc[1] * res + gc[2] * res * res) % 2 ** 32
            else:
                idx = gc[0] ^ (gc[1] * int(PRIME1) % 2 ** 32) ^ (gc[2] * int(PRIME2) % 2 ** 32)
            idx %= size
            wt = [w[k] if d[k] else ft(1) - w[k] for k in range(3)]
            weight = (wt[0] * wt[1]) * wt[2]
            for f in range(FEATURES):
                out[n, f] = out[n, f] + weight * g[off + idx, f]
    return torch.from_numpy(out)


def encode_backward(x, denc, lay, mask=None):
    """dgrid [offset_L F] of ``denc``'s dtype"""
    u, ok = _unit(x, denc.dtype, mask)
    denc = torch.where(ok[:, None], denc, torch.zeros_like(denc))
    dgrid = torch.zeros(int(lay["offset"][-1]), FEATURES, dtype=denc.dtype)
    for l in range(lay["num_levels"]):
        for idx, wt in _cells(u, lay, l):
            dgrid.index_add_(0, int(lay["offset"][l]) + idx, wt[:, None] * denc[:, FEATURES * l:FEATURES * (l + 1)])
    return dgrid.view(-1)


def mlp(enc, w1, b1, w2, b2):
    return torch.relu(enc @ w1.T + b1) @ w2.T + b2


def field(x, grid, w1, b1, w2, b2, lay, mask=None):
    """color [N,3]"""
    color = torch.sigmoid(mlp(encode(x, grid, lay, mask), w1, b1, w2, b2))
    return torch.where(valid_rows(x, mask)[:, None], color, torch.zeros_like(color))


def _sum_points(terms, sequential):
    """sum over the first axis: torch's, or one point after the other (cumsum is sequential on the CPU)"""
    return torch.cumsum(terms, 0)[-1] if sequential else terms.sum(0)


def field_backward(x, grid, w1, b1, w2, b2, lay, dcolor, mask=None, order=None, sequential=False):
    """dict(color, dgrid, dw1, db1, dw2, db2) from the header's formulas; ``order``: a permutation of the points;
    ``sequential``: the four MLP gradients as plain running sums over the points in that order (``dgrid`` always is one:
    ``index_add_`` on the CPU walks its rows in order)"""
    n = x.shape[0]
    perm = torch.arange(n) if order is None else torch.as_tensor(order)
    xp, dc = x[perm], dcolor[perm].to(grid.dtype)
    mp = None if mask is None else mask[perm]
    ok = valid_rows(xp.to(grid.dtype), mp)
    enc = encode(xp, grid, lay, mp)
    z = enc @ w1.T + b1
    h = torch.relu(z)
    color = torch.where(ok[:, None], torch.sigmoid(h @ w2.T + b2), torch.zeros(n, 3, dtype=grid.dtype))
    do = (dc * color) * (1 - color)
    dh = (do @ w2) * (h > 0)
    if sequential:
        out = dict(dw2=_sum_points(do[:, :, None] * h[:, None, :], True), dw1=_sum_points(dh[:, :, None] * enc[:, None, :], True))
    else:
        out = dict(dw2=do.T @ h, dw1=dh.T @ enc)
    out.update(db2=_sum_points(do, sequential), db1=_sum_points(dh, sequential), dgrid=encode_backward(xp, dh @ w1, lay, mp))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    out["color"] = color[inv]
    return out


def sample_points(n, seed=0):
    """float32 [n,3] of the test plan: uniform in [-1, 1]^3, then (where n allows) rows of exact -1 / 0 / +1 coordinates, a
    row at -1.5 and one at 2.0, one NaN row and one inf row"""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    special = [[-1, -1, -1], [0, 0, 0], [1, 1, 1], [-1, 0, 1], [1, 0.25, -1], [-1.5, 0.3, -1.5], [2.0, 2.0, -0.7],
               [np.nan, 0.1, 0.2], [0.5, np.inf, -0.5]]
    for k, row in enumerate(special):
        if 2 * k + 1 < n:
            x[2 * k + 1] = row
    return torch.from_numpy(x)
