"""numpy statement of include/gd_sample.h: the screen-space derivatives of (u, v) and of interpolated attributes, the mip
pyramid, the four filter modes with wrap / clamp, and the gradient to the texture by sequential sums.  Every function takes
``dtype``: float32 follows the header operation by operation (one rounding each, its order), float64 is the same
arithmetic in double, the reference of the tests that carry a tolerance.  ``render_mesh`` restates the package's textured
render over tests/mesh_reference.py.  Test infrastructure: never imported by the package."""
import numpy as np

NEAREST, LINEAR, LINEAR_MIPMAP_NEAREST, LINEAR_MIPMAP_LINEAR = 0, 1, 2, 3
FILTERS = {"nearest": 0, "linear": 1, "linear-mipmap-nearest": 2, "linear-mipmap-linear": 3}
WRAP, CLAMP = 0, 1
BOUNDARIES = {"wrap": 0, "clamp": 1}
TAPS = {0: 1, 1: 4, 2: 4, 3: 8}


# ---- (a) rast_db, (b) attribute derivatives ---------------------------------------------------------------------------

def rast_db(rast, pos, tri, dtype=np.float32):
    """[H,W,4] = (du/dX, du/dY, dv/dX, dv/dY)"""
    f = dtype
    H, W = rast.shape[:2]
    pos = np.asarray(pos, dtype=np.float32).astype(f)
    tri = np.asarray(tri, dtype=np.int64)
    V, F = pos.shape[0], tri.shape[0]
    out = np.zeros((H, W, 4), dtype=f)
    ids = rast[..., 3]
    with np.errstate(all="ignore"):
        for r in range(H):
            for c in range(W):
                idf = ids[r, c]
                if not (idf >= 1 and idf <= F):
                    continue
                i = tri[int(idf) - 1]
                if (i < 0).any() or (i >= V).any():
                    continue
                P = pos[i]
                fx = f(2 * c + 1) / f(W) - f(1)
                fy = f(2 * r + 1) / f(H) - f(1)
                qx = P[:, 0] - fx * P[:, 3]
                qy = P[:, 1] - fy * P[:, 3]
                w = P[:, 3]
                a0 = qx[1] * qy[2] - qy[1] * qx[2]
                a1 = qx[2] * qy[0] - qy[2] * qx[0]
                a2 = qx[0] * qy[1] - qy[0] * qx[1]
                s = (a0 + a1) + a2
                if s == 0 or not np.isfinite(s):
                    continue
                da0x, da1x, da2x = qy[1] * w[2] - w[1] * qy[2], qy[2] * w[0] - w[2] * qy[0], qy[0] * w[1] - w[0] * qy[1]
                da0y, da1y, da2y = w[1] * qx[2] - qx[1] * w[2], w[2] * qx[0] - qx[2] * w[0], w[0] * qx[1] - qx[0] * w[1]
                dsx, dsy = (da0x + da1x) + da2x, (da0y + da1y) + da2y
                ss = s * s
                ux, uy = (da0x * s - a0 * dsx) / ss, (da0y * s - a0 * dsy) / ss
                vx, vy = (da1x * s - a1 * dsx) / ss, (da1y * s - a1 * dsy) / ss
                kx, ky = f(2) / f(W), f(2) / f(H)
                out[r, c] = (ux * kx, uy * ky, vx * kx, vy * ky)
    return out


def ideal_uv_at(pos3, X, Y, H, W):
    """float64 (u, v) of the header's unsnapped rasterize for the triangle ``pos3`` [3,4] at the CONTINUOUS pixel position
    (X, Y) (the centre of pixel (r, c) is X = c + 0.5, Y = r + 0.5): what rast_db differentiates"""
    P = np.asarray(pos3, dtype=np.float64)
    fx, fy = 2.0 * X / W - 1.0, 2.0 * Y / H - 1.0
    qx, qy = P[:, 0] - fx * P[:, 3], P[:, 1] - fy * P[:, 3]
    a0 = qx[1] * qy[2] - qy[1] * qx[2]
    a1 = qx[2] * qy[0] - qy[2] * qx[0]
    a2 = qx[0] * qy[1] - qy[0] * qx[1]
    s = a0 + a1 + a2
    return a0 / s, a1 / s


def interpolate_da(attr, rast, db, tri, dtype=np.float32):
    """[H,W,2C]"""
    f = dtype
    attr = np.asarray(attr, dtype=np.float32).astype(f)
    tri = np.asarray(tri, dtype=np.int64)
    V, C = attr.shape
    F = tri.shape[0]
    H, W = rast.shape[:2]
    db = np.asarray(db).astype(f)
    out = np.zeros((H, W, 2 * C), dtype=f)
    ids = rast[..., 3]
    ok = (ids >= 1) & (ids <= F)
    t = tri[np.where(ok, ids, 1).astype(np.int64) - 1]                    # [H,W,3]
    ok &= ((t >= 0) & (t < V)).all(axis=-1)
    t = np.clip(t, 0, V - 1)
    e0 = attr[t[..., 0]] - attr[t[..., 2]]
    e1 = attr[t[..., 1]] - attr[t[..., 2]]
    with np.errstate(all="ignore"):
        dx = db[..., 0:1] * e0 + db[..., 2:3] * e1
        dy = db[..., 1:2] * e0 + db[..., 3:4] * e1
    out[..., 0::2] = np.where(ok[..., None], dx, 0)
    out[..., 1::2] = np.where(ok[..., None], dy, 0)
    return out


# ---- (c) the pyramid --------------------------------------------------------------------------------------------------

def pyramid_shapes(Ht, Wt, max_mip_level=None):
    """[(Hl, Wl)] for levels 0 .. L"""
    full = int(np.floor(np.log2(max(Ht, Wt))))
    top = full if max_mip_level is None else min(int(max_mip_level), full)
    if top > 0 and ((Ht & (Ht - 1)) or (Wt & (Wt - 1))):
        raise ValueError("mip levels need power-of-two sides")
    return [(max(Ht >> l, 1), max(Wt >> l, 1)) for l in range(top + 1)]


def build_mips(tex, max_mip_level=None, dtype=np.float32):
    """the list of levels, each [Hl,Wl,C]"""
    f = dtype
    levels = [np.asarray(tex).astype(f)]
    for (Hl, Wl) in pyramid_shapes(tex.shape[0], tex.shape[1], max_mip_level)[1:]:
        p = levels[-1]
        Hp, Wp = p.shape[:2]
        if Wp > 1 and Hp > 1:
            a, b, c, d = p[0::2, 0::2], p[0::2, 1::2], p[1::2, 0::2], p[1::2, 1::2]
            nxt = ((a + b) + (c + d)) * f(0.25)
        elif Wp == 1:
            nxt = (p[0::2] + p[1::2]) * f(0.5)
        else:
            nxt = (p[:, 0::2] + p[:, 1::2]) * f(0.5)
        assert nxt.shape[:2] == (Hl, Wl)
        levels.append(nxt.astype(f))
    return levels


def offsets(levels):
    """first texel of each level in the one buffer, then the total"""
    return np.concatenate(([0], np.cumsum([lv.shape[0] * lv.shape[1] for lv in levels]))).astype(np.int64)


# ---- (d) sampling -----------------------------------------------------------------------------------------------------

def _index(i, n, boundary):
    k = np.clip(i, -2.0 ** 30, 2.0 ** 30).astype(np.int64)
    return np.clip(k, 0, n - 1) if boundary == CLAMP else np.mod(k, n)


def _taps(shape, u, v, boundary, f):
    """(rows [N,4], columns [N,4], fx, fy) in the order 00, 10, 01, 11"""
    Hl, Wl = shape
    xs, ys = u * f(Wl), v * f(Hl)
    x0, y0 = np.floor(xs - f(0.5)), np.floor(ys - f(0.5))
    fx, fy = (xs - x0) - f(0.5), (ys - y0) - f(0.5)
    c0, c1 = _index(x0, Wl, boundary), _index(x0 + f(1), Wl, boundary)
    r0, r1 = _index(y0, Hl, boundary), _index(y0 + f(1), Hl, boundary)
    return np.stack((r0, r0, r1, r1), 1), np.stack((c0, c1, c0, c1), 1), fx, fy


def _bilinear(level, u, v, boundary, f):
    rows, cols, fx, fy = _taps(level.shape[:2], u, v, boundary, f)
    t = level[rows, cols]                                                 # [N,4,C]
    fx, fy = fx[:, None], fy[:, None]
    p = t[:, 0] + fx * (t[:, 1] - t[:, 0])
    q = t[:, 2] + fx * (t[:, 3] - t[:, 2])
    return p + fy * (q - p)


def mip_level(uv_da, Ht, Wt, L, dtype=np.float32):
    f = dtype
    da = np.asarray(uv_da).astype(f)
    with np.errstate(all="ignore"):
        sx, sy, tx, ty = da[:, 0] * f(Wt), da[:, 1] * f(Wt), da[:, 2] * f(Ht), da[:, 3] * f(Ht)
        A, B, Cc = sx * sx + tx * tx, sy * sy + ty * ty, sx * sy + tx * ty
        d = A - B
        m = f(0.5) * (A + B) + np.sqrt(f(0.25) * (d * d) + Cc * Cc)
        good = (m > 0) & np.isfinite(m)
        level = f(0.5) * np.log2(np.where(good, m, 1)).astype(f)
    return np.where(good, np.minimum(np.maximum(level, f(0)), f(L)), f(0)).astype(f)


def _pick_levels(filter_id, uv_da, Ht, Wt, L, f, n):
    """(l0, l1, frac): int arrays and the blend factor (0 where one level is sampled)"""
    if filter_id < LINEAR_MIPMAP_NEAREST:
        z = np.zeros(n, dtype=np.int64)
        return z, z, np.zeros(n, dtype=f)
    level = mip_level(uv_da, Ht, Wt, L, f)
    if filter_id == LINEAR_MIPMAP_NEAREST:
        l = np.floor(level + f(0.5)).astype(np.int64)
        return l, l, np.zeros(n, dtype=f)
    fl = np.floor(level)
    l0 = fl.astype(np.int64)
    return l0, np.minimum(l0 + 1, L), (level - fl).astype(f)


def texture(levels, uv, uv_da=None, filter_id=LINEAR, boundary=WRAP, dtype=np.float32):
    """out [N,C] of the pyramid ``levels`` (``build_mips`` in the same dtype) at uv [N,2]"""
    f = dtype
    uv = np.asarray(uv, dtype=np.float32)
    N, C = uv.shape[0], levels[0].shape[2]
    Ht, Wt = levels[0].shape[:2]
    L = len(levels) - 1
    fin = np.isfinite(uv).all(axis=1)
    u, v = np.where(fin, uv[:, 0], 0).astype(f), np.where(fin, uv[:, 1], 0).astype(f)
    with np.errstate(all="ignore"):
        if filter_id == NEAREST:
            out = levels[0][_index(np.floor(v * f(Ht)), Ht, boundary), _index(np.floor(u * f(Wt)), Wt, boundary)]
        else:
            l0, l1, frac = _pick_levels(filter_id, uv_da, Ht, Wt, L, f, N)
            out = np.zeros((N, C), dtype=f)
            for l in range(L + 1):
                sel = np.flatnonzero(l0 == l)
                if sel.size:
                    out[sel] = _bilinear(levels[l], u[sel], v[sel], boundary, f)
            for l in range(L + 1):
                sel = np.flatnonzero((l1 == l) & (frac != 0))
                if sel.size:
                    c1 = _bilinear(levels[l], u[sel], v[sel], boundary, f)
                    out[sel] = out[sel] + frac[sel, None] * (c1 - out[sel])
    return np.where(fin[:, None], out, 0).astype(f)


# ---- (e) the gradient to the texture ----------------------------------------------------------------------------------

def texture_items(shapes, uv, uv_da, dout, filter_id, boundary, dtype=np.float32):
    """(keys int64 [N T], values [N T, C]) in item order; the key of a dropped item is the pyramid's total"""
    f = dtype
    uv = np.asarray(uv, dtype=np.float32)
    dout = np.asarray(dout).astype(f)
    N, C, T = uv.shape[0], dout.shape[1], TAPS[filter_id]
    off = np.concatenate(([0], np.cumsum([h * w for h, w in shapes]))).astype(np.int64)
    Ht, Wt = shapes[0]
    L = len(shapes) - 1
    fin = np.isfinite(uv).all(axis=1)
    u, v = np.where(fin, uv[:, 0], 0).astype(f), np.where(fin, uv[:, 1], 0).astype(f)
    keys = np.full((N, T), off[-1], dtype=np.int64)
    vals = np.zeros((N, T, C), dtype=f)
    with np.errstate(all="ignore"):
        if filter_id == NEAREST:
            keys[:, 0] = _index(np.floor(v * f(Ht)), Ht, boundary) * Wt + _index(np.floor(u * f(Wt)), Wt, boundary)
            vals[:, 0] = dout
        else:
            l0, l1, frac = _pick_levels(filter_id, uv_da, Ht, Wt, L, f, N)
            two = (filter_id == LINEAR_MIPMAP_LINEAR) & (frac != 0)
            for which, lv, lw in ((0, l0, f(1) - frac), (1, l1, frac)):
                if which == 1 and T != 8:
                    break
                for l in range(L + 1):
                    sel = np.flatnonzero((lv == l) & (two if which == 1 else True))
                    if not sel.size:
                        continue
                    rows, cols, fx, fy = _taps(shapes[l], u[sel], v[sel], boundary, f)
                    gx, gy = f(1) - fx, f(1) - fy
                    w = np.stack((gx * gy, fx * gy, gx * fy, fx * fy), 1)             # [n,4]
                    w = np.where(two[sel, None], lw[sel, None] * w, w)
                    keys[sel, 4 * which:4 * which + 4] = off[l] + rows * shapes[l][1] + cols
                    vals[sel, 4 * which:4 * which + 4] = w[:, :, None] * dout[sel, None, :]
    keys[~fin] = off[-1]
    vals[~fin] = 0
    return keys.reshape(-1), vals.reshape(N * T, C).astype(f)


def texture_backward(shapes, uv, uv_da, dout, filter_id, boundary, dtex, dtype=np.float32):
    """``dtex`` [Ht,Wt,C] plus the gradient, by the header's steps: items, stable sort, sequential sums from +0, the fold
    from the top level down, one add per texel where the folded gradient is not 0"""
    f = dtype
    keys, vals = texture_items(shapes, uv, uv_da, dout, filter_id, boundary, f)
    C = vals.shape[1]
    off = np.concatenate(([0], np.cumsum([h * w for h, w in shapes]))).astype(np.int64)
    g = np.zeros((off[-1], C), dtype=f)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    live = sk < off[-1]
    order, sk = order[live], sk[live]
    with np.errstate(all="ignore"):
        if sk.size:
            starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
            ends = np.r_[starts[1:], sk.size]
            run = (ends - starts).max()
            acc = np.zeros((starts.size, C), dtype=f)
            for step in range(run):                                           # the step-th item of every run, in order
                has = starts + step < ends
                acc[has] = acc[has] + vals[order[starts[has] + step]]
            g[sk[starts]] = acc
        L = len(shapes) - 1
        for l in range(L - 1, -1, -1):
            Hl, Wl = shapes[l]
            Hp, Wp = shapes[l + 1]
            w = f(0.25) if (Wl > 1 and Hl > 1) else f(0.5)
            fine = g[off[l]:off[l + 1]].reshape(Hl, Wl, C)
            coarse = g[off[l + 1]:off[l + 2]].reshape(Hp, Wp, C)
            y, x = np.arange(Hl) >> 1, np.arange(Wl) >> 1
            fine += w * coarse[y[:, None], x[None, :]]
        Ht, Wt = shapes[0]
        g0 = g[:Ht * Wt].reshape(Ht, Wt, C)
        base = np.asarray(dtex).astype(f)
        return np.where(g0 != 0, base + g0, base).astype(f)


# ---- the textured render ----------------------------------------------------------------------------------------------

def render_mesh(mref, pos, v_cam, tri, vt, ft, albedo, vn, pose, H, W, filter_name, boundary_name, bg=1.0, vc=None, cache=None):
    """float64 dict of the package's ``render_mesh`` over tests/mesh_reference.py (``mref``): rast, the antialias
    weights and the interpolated uv are its fp32 statements (the kernels equal them bit for bit), everything after them
    is float64.  ``pos`` / ``v_cam``: the clip- and camera-space positions the package formed (a last-bit difference in a
    position can move a snapped vertex)."""
    pos, v_cam = np.ascontiguousarray(pos, dtype=np.float32), np.asarray(v_cam, dtype=np.float32)
    if cache is None or (H, W) not in cache:                              # ``cache``: a dict shared by renders of one camera
        rast = mref.rasterize(pos, tri, H, W)
        made = (rast, mref.antialias_weights(rast, pos, tri, mref.build_opposite(tri)).astype(np.float64))
        if cache is not None:
            cache[(H, W)] = made
    rast, wts = made if cache is None else cache[(H, W)]
    r64 = rast.astype(np.float64)
    ids = rast[..., 3].astype(np.int64)
    hit = ids > 0

    def interp(attr, faces):
        a = np.asarray(attr, dtype=np.float32).astype(np.float64)
        t = np.asarray(faces, dtype=np.int64)[np.maximum(ids - 1, 0)]
        u, w_ = r64[..., 0:1], r64[..., 1:2]
        out = (u * a[t[..., 0]] + w_ * a[t[..., 1]]) + ((1 - u) - w_) * a[t[..., 2]]
        return np.where(hit[..., None], out, 0.0)

    def aa(x):
        acc = x.astype(np.float64)
        for k, nb in enumerate(mref._neighbours(x.astype(np.float64))):
            acc = acc + wts[..., k:k + 1] * (nb - x)
        return acc

    alpha = np.clip(aa(hit[..., None].astype(np.float64)), 0, 1)
    depth = interp(-v_cam[:, 2:3], tri)
    if vc is not None:
        color = interp(vc, tri)
    else:
        # uv is an fp32 quantity (gd_mesh.h's interpolate, which the kernel equals bit for bit): the sampler's input, not
        # a result under test here
        texc = mref.interpolate(vt, rast, ft).reshape(-1, 2)
        fid, bid = FILTERS[filter_name], BOUNDARIES[boundary_name]
        da = None
        if fid >= LINEAR_MIPMAP_NEAREST:
            da = interpolate_da(vt, rast, rast_db(rast, pos, tri, np.float64), ft, np.float64).reshape(-1, 4)
        levels = build_mips(np.asarray(albedo, dtype=np.float64) / 255.0 if albedo.dtype == np.uint8 else albedo,
                            None if fid >= LINEAR_MIPMAP_NEAREST else 0, np.float64)
        color = texture(levels, texc, da, fid, bid, np.float64).reshape(H, W, 3)
    color = aa(color)
    image = np.clip(alpha * color + (1 - alpha) * bg, 0, 1)
    n = interp(vn, tri)
    n = n / np.sqrt(np.maximum((n * n).sum(-1, keepdims=True), 1e-20))
    viewcos = (n @ np.asarray(pose, dtype=np.float64)[:3, :3])[..., 2:3]
    return {"image": image, "alpha": alpha, "depth": depth, "normal": (n + 1) / 2, "viewcos": viewcos}
