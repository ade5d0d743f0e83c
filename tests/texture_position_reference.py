"""The definition of include/gd_texture_position.h in torch on the CPU, by dtype: the REFERENCE of the tests of the texture
field's gradient to the sample positions.  A statement of its own: ``texture_reference._unit`` detaches ``x``, so the cells
are formed here again, from the header's text.

  * ``position_gradient(x, grid, denc, lay, mask)``   the closed form, ``dx`` [N,3] of ``grid``'s dtype.  In float32 every
    operation is one IEEE operation in the header's order (torch's CPU kernels do not fuse a multiply into an add), so it
    is what the GPU must return bit for bit; in float64 it is the measure.
  * ``encode_autograd(x, grid, lay, mask)``           the encoding with ``x`` NOT detached: autograd differentiates the
    interpolation weights, ``floor`` passes no gradient
  * ``field_position_gradient(x, p, lay, dcolor, mask)``   ``dx`` of the fused field: ``denc`` from gd_texture.h's backward
    formulas in the dtype of the parameters, then the closed form
  * ``interior(x, lay, margin)``                      the points whose fractional part is at least ``margin`` away from a
    cell wall on every level and axis (float64), where central differences see one cell
"""
import numpy as np
import torch

from tests import texture_reference as tref

FEATURES = tref.FEATURES


def _stand_in(x, dtype, mask):
    """(x with a finite stand-in on the rows that take no part, which rows take part)"""
    x = x.to(dtype)
    ok = tref.valid_rows(x.detach(), mask)
    return torch.where(ok[:, None], x, torch.zeros_like(x)), ok


def _cell(u, scale):
    """(c uint32 numpy [N,3], w [N,3]) of unit-cube coordinates ``u``; ``w`` carries ``u``'s autograd history"""
    p = u * float(scale)
    p = p + 0.5
    fl = torch.floor(p.detach())
    return fl.to(torch.int32).numpy().view(np.uint32), p - fl


def _corner_index(c, i, lay, l):
    """int64 tensor [N]: the entry of corner ``i`` in the whole table"""
    res, size = np.uint32(lay["res"][l]), np.uint32(lay["size"][l])
    with np.errstate(over="ignore"):
        g = [c[:, k] + np.uint32((i >> k) & 1) for k in range(3)]
        if lay["dense"][l]:
            idx = g[0] + g[1] * res + g[2] * res * res
        else:
            idx = g[0] ^ (g[1] * tref.PRIME1) ^ (g[2] * tref.PRIME2)
        idx = idx % size
    return torch.from_numpy(idx.astype(np.int64)) + int(lay["offset"][l])


def position_gradient(x, grid, denc, lay, mask=None):
    """dx [N,3] of ``grid``'s dtype, the header's operations in the header's order"""
    dt = grid.dtype
    xs, ok = _stand_in(x.detach(), dt, mask)
    u = (xs + 1) * 0.5
    table = grid.detach().view(-1, FEATURES)
    denc = denc.to(dt)
    dx = torch.zeros(x.shape[0], 3, dtype=dt)
    for l in range(lay["num_levels"]):
        c, w = _cell(u, lay["scale"][l])
        S = [torch.zeros(x.shape[0], dtype=dt) for _ in range(3)]
        for i in range(8):
            g = table[_corner_index(c, i, lay, l)]
            wt = [w[:, k] if (i >> k) & 1 else 1 - w[:, k] for k in range(3)]
            t = denc[:, 2 * l] * g[:, 0] + denc[:, 2 * l + 1] * g[:, 1]
            q = [(wt[1] * wt[2]) * t, (wt[0] * wt[2]) * t, (wt[0] * wt[1]) * t]
            for d in range(3):
                S[d] = S[d] + q[d] if (i >> d) & 1 else S[d] - q[d]
        k = torch.tensor(0.5, dtype=dt) * torch.tensor(float(lay["scale"][l]), dtype=dt)
        dx = dx + k * torch.stack(S, dim=1)
    return torch.where(ok[:, None], dx, torch.zeros_like(dx))


def encode_autograd(x, grid, lay, mask=None):
    """[N, L F] of ``grid``'s dtype, differentiable in ``x`` (and in ``grid``)"""
    xs, ok = _stand_in(x, grid.dtype, mask)
    u = (xs + 1) * 0.5
    table = grid.view(-1, FEATURES)
    cols = []
    for l in range(lay["num_levels"]):
        c, w = _cell(u, lay["scale"][l])
        acc = torch.zeros(x.shape[0], FEATURES, dtype=grid.dtype)
        for i in range(8):
            wt = [w[:, k] if (i >> k) & 1 else 1 - w[:, k] for k in range(3)]
            acc = acc + ((wt[0] * wt[1]) * wt[2])[:, None] * table[_corner_index(c, i, lay, l)]
        cols.append(acc)
    enc = torch.cat(cols, dim=1)
    return torch.where(ok[:, None], enc, torch.zeros_like(enc))


def field_denc(x, p, lay, dcolor, mask=None):
    """denc [N,32] = W1^T dh of gd_texture.h's backward, in the dtype of the parameters ``p`` (grid, w1, b1, w2, b2)"""
    dt = p["grid"].dtype
    ok = tref.valid_rows(x.to(dt), mask)
    enc = tref.encode(x, p["grid"], lay, mask)
    h = torch.relu(enc @ p["w1"].T + p["b1"])
    color = torch.where(ok[:, None], torch.sigmoid(h @ p["w2"].T + p["b2"]), torch.zeros(x.shape[0], 3, dtype=dt))
    do = (dcolor.to(dt) * color) * (1 - color)
    return ((do @ p["w2"]) * (h > 0)) @ p["w1"]


def field_position_gradient(x, p, lay, dcolor, mask=None):
    return position_gradient(x, p["grid"], field_denc(x, p, lay, dcolor, mask), lay, mask)


def interior(x, lay, margin=1e-3):
    """bool [N]: finite, and on every level and axis the fractional part (float64) lies in [margin, 1 - margin]"""
    ok = torch.isfinite(x).all(dim=1)
    u = (torch.where(ok[:, None], x, torch.zeros_like(x)).double() + 1) * 0.5
    for l in range(lay["num_levels"]):
        _, w = _cell(u, lay["scale"][l])
        ok = ok & ((w >= margin) & (w <= 1 - margin)).all(dim=1)
    return ok


def rel(got, want64):
    """the project's measure: max|g - g64| / max|g64|"""
    return float((got.detach().cpu().double().reshape(want64.shape) - want64).abs().max() / want64.abs().max())
