"""numpy statement of the mesh render path (include/gd_mesh.h: rasterize, interpolate, antialias): the checker of
tests/test_mesh_render_*.py.  fp32 with one rounding per operation in the order the header states, edges in int64, every
triangle tested against every pixel.  Test infrastructure: never imported by the package.

The only concession to size is ``window``: triangles whose (generously padded) pixel box fits a ``window`` x ``window``
patch are tested against that patch only, all such triangles in one vectorised step; pixels outside a triangle's box
cannot be covered by it, so the result is the same as testing the whole frame.  ``window=0`` tests the whole frame."""
import numpy as np

F32 = np.float32
SNAP_LIMIT = 1 << 24
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def snap_vertices(pos, H, W):
    """(ok [V] bool, X [V] int64, Y [V] int64, zn [V] f32, rw [V] f32); values of unusable vertices are zero."""
    pos = np.ascontiguousarray(pos, dtype=F32)
    with np.errstate(all="ignore"):
        w = pos[:, 3]
        rw = F32(1.0) / w
        xn, yn, zn = pos[:, 0] * rw, pos[:, 1] * rw, pos[:, 2] * rw
        fx = np.rint((xn * F32(0.5) + F32(0.5)) * F32(256 * W))
        fy = np.rint((yn * F32(0.5) + F32(0.5)) * F32(256 * H))
        assert fx.dtype == F32 and zn.dtype == F32
        ok = (w > 0) & np.isfinite(rw) & np.isfinite(xn) & np.isfinite(yn) & np.isfinite(zn)
        ok &= (np.abs(fx) <= F32(SNAP_LIMIT)) & (np.abs(fy) <= F32(SNAP_LIMIT))      # NaN compares false
    X = np.where(ok, fx, 0).astype(np.int64)
    Y = np.where(ok, fy, 0).astype(np.int64)
    return ok, X, Y, np.where(ok, zn, F32(0)).astype(F32), np.where(ok, rw, F32(0)).astype(F32)


def _setup(pos, tri, H, W):
    """Per usable triangle: index, corner X Y zn rw [n,3], normalised edge vectors dX dY [n,3], A [n] > 0."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    V = pos.shape[0]
    ok, X, Y, zn, rw = snap_vertices(pos, H, W)
    inrange = np.all((tri >= 0) & (tri < V), axis=1)
    t = np.clip(tri, 0, max(V - 1, 0))
    usable = inrange & np.all(ok[t], axis=1) if V else np.zeros(tri.shape[0], bool)
    idx = np.flatnonzero(usable)
    t = t[idx]
    tx, ty = X[t], Y[t]
    j, k = [1, 2, 0], [2, 0, 1]
    dX, dY = tx[:, k] - tx[:, j], ty[:, k] - ty[:, j]
    A = dX[:, 0] * (ty[:, 0] - ty[:, 1]) - dY[:, 0] * (tx[:, 0] - tx[:, 1])
    keep = A != 0
    idx, tx, ty, dX, dY, A, t = idx[keep], tx[keep], ty[keep], dX[keep], dY[keep], A[keep], t[keep]
    neg = A < 0
    dX[neg], dY[neg], A[neg] = -dX[neg], -dY[neg], -A[neg]
    return dict(idx=idx, X=tx, Y=ty, zn=zn[t], rw=rw[t], dX=dX, dY=dY, A=A)


def _depth_bits(zw):
    b = zw.view(np.uint32).astype(np.uint64)
    return np.where(b & np.uint64(0x80000000), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))


def _evaluate(s, sel, rows, cols):
    """Triangles ``sel`` of setup ``s`` at pixels rows / cols (broadcastable to [n, ...]).  Returns (valid, u, v, zw)."""
    n = len(sel)
    shp = (n,) + (1,) * (max(np.ndim(rows), np.ndim(cols)) - 1)      # rows / cols: [n or 1, ...]
    Px = 256 * np.asarray(cols, dtype=np.int64) + 128
    Py = 256 * np.asarray(rows, dtype=np.int64) + 128
    jn = [1, 2, 0]
    E, cov = [], True
    for i in range(3):
        dX, dY = s["dX"][sel, i].reshape(shp), s["dY"][sel, i].reshape(shp)
        e = dX * (Py - s["Y"][sel, jn[i]].reshape(shp)) - dY * (Px - s["X"][sel, jn[i]].reshape(shp))
        cov = cov & ((e > 0) | ((e == 0) & ((dY > 0) | ((dY == 0) & (dX < 0)))))
        E.append(e)
    with np.errstate(all="ignore"):
        fa = s["A"][sel].reshape(shp).astype(F32)
        b = [e.astype(F32) / fa for e in E]
        zn = [s["zn"][sel, i].reshape(shp) for i in range(3)]
        rw = [s["rw"][sel, i].reshape(shp) for i in range(3)]
        zw = (b[0] * zn[0] + b[1] * zn[1]) + b[2] * zn[2]
        zw = np.where(zw == 0, F32(0), zw).astype(F32)
        p = [b[i] * rw[i] for i in range(3)]
        ssum = (p[0] + p[1]) + p[2]
        u, v = p[0] / ssum, p[1] / ssum
        assert zw.dtype == F32 and u.dtype == F32
        valid = cov & (zw >= F32(-1)) & (zw <= F32(1))
    return valid, u, v, zw


def rasterize(pos, tri, H, W, window=0):
    """rast [H,W,4] fp32 = (u, v, zw, id + 1) by the definition of include/gd_mesh.h."""
    pos = np.ascontiguousarray(pos, dtype=F32)
    s = _setup(pos, tri, H, W)
    n = len(s["idx"])
    key = np.full(H * W, EMPTY, dtype=np.uint64)

    def commit(valid, zw, ids, pix):
        k = (_depth_bits(zw[valid]) << np.uint64(32)) | ids[valid].astype(np.uint64)
        np.minimum.at(key, pix[valid], k)

    whole = np.arange(n)
    chunk = max(1, (1 << 21) // (H * W))                              # triangles per whole-frame step
    if window and n:
        # generous box: two pixels wider than the vertices on every side
        c_lo = (s["X"].min(axis=1) >> 8) - 2
        r_lo = (s["Y"].min(axis=1) >> 8) - 2
        fits = ((s["X"].max(axis=1) >> 8) + 2 - c_lo < window) & ((s["Y"].max(axis=1) >> 8) + 2 - r_lo < window)
        sel = np.flatnonzero(fits)
        whole = np.flatnonzero(~fits)
        for a in range(0, len(sel), 4096):
            part = sel[a:a + 4096]
            rows = r_lo[part][:, None, None] + np.arange(window)[None, :, None]
            cols = c_lo[part][:, None, None] + np.arange(window)[None, None, :]
            rows, cols = np.broadcast_arrays(rows, cols)
            valid, _, _, zw = _evaluate(s, part, rows, cols)
            valid = valid & (rows >= 0) & (rows < H) & (cols >= 0) & (cols < W)
            ids = np.broadcast_to(s["idx"][part][:, None, None], valid.shape)
            commit(valid, zw, ids, rows * W + cols)
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for a in range(0, len(whole), chunk):
        part = whole[a:a + chunk]
        valid, _, _, zw = _evaluate(s, part, rr[None], cc[None])
        ids = np.broadcast_to(s["idx"][part][:, None, None], valid.shape)
        commit(valid, zw, ids, np.broadcast_to((rr * W + cc)[None], valid.shape))
    # decode the winners and recompute their values
    rast = np.zeros((H * W, 4), dtype=F32)
    hit = np.flatnonzero(key != EMPTY)
    if len(hit):
        ids = (key[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        where = np.full(int(s["idx"].max()) + 1, -1, dtype=np.int64)
        where[s["idx"]] = np.arange(n)
        valid, u, v, zw = _evaluate(s, where[ids], hit // W, hit % W)
        assert valid.all()
        rast[hit] = np.stack((u, v, zw, (ids + 1).astype(F32)), axis=1)
    return rast.reshape(H, W, 4)


def interpolate(attr, rast, tri):
    """out [H,W,C] fp32 = (u a0 + v a1) + ((1 - u) - v) a2; 0 on background."""
    attr = np.ascontiguousarray(attr, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    ids = rast[..., 3].astype(np.int64)
    t = tri[np.maximum(ids - 1, 0)]
    u, v = rast[..., 0:1], rast[..., 1:2]
    w = (F32(1) - u) - v
    out = (u * attr[t[..., 0]] + v * attr[t[..., 1]]) + w * attr[t[..., 2]]
    assert out.dtype == F32
    return np.where((ids > 0)[..., None], out, F32(0)).astype(F32)


def interpolate_backward_terms(dout, rast, tri, V):
    """(sum [V,C] float64, sum of |terms| [V,C] float64) of the attribute gradient."""
    tri = np.asarray(tri, dtype=np.int64)
    ids = rast[..., 3].astype(np.int64).ravel()
    hit = np.flatnonzero(ids > 0)
    t = tri[ids[hit] - 1]
    u, v = rast[..., 0].ravel()[hit], rast[..., 1].ravel()[hit]
    w = (F32(1) - u) - v
    d = dout.reshape(-1, dout.shape[-1])[hit].astype(np.float64)
    total = np.zeros((V, d.shape[1]))
    mag = np.zeros((V, d.shape[1]))
    for i, wt in enumerate((u, v, w)):
        term = wt.astype(np.float64)[:, None] * d
        np.add.at(total, t[:, i], term)
        np.add.at(mag, t[:, i], np.abs(term))
    return total, mag


def build_opposite(tri):
    """opp [F,3] int32: the vertex across edge i (opposite vertex i) in the one other triangle on that edge; -1 if the
    edge has != 2 triangles.  A plain dictionary walk, independent of the package's numpy version."""
    tri = np.asarray(tri, dtype=np.int64)
    edges = {}
    for t, (a, b, c) in enumerate(tri):
        for i, (p, q, o) in enumerate(((b, c, a), (c, a, b), (a, b, c))):
            edges.setdefault((min(p, q), max(p, q)), []).append((t, i, o))
    opp = np.full(tri.shape, -1, dtype=np.int32)
    for users in edges.values():
        if len(users) == 2:
            (t0, i0, o0), (t1, i1, o1) = users
            opp[t0, i0], opp[t1, i1] = o1, o0
    return opp


def antialias_weights(rast, pos, tri, opp, info=None):
    """wts [H,W,4] fp32, k = (left, right, row - 1, row + 1), by the definition of include/gd_mesh.h.  ``info`` (a dict)
    receives counts of the weights by kind: to_outer, to_inner, horizontal, vertical, fold, boundary."""
    H, W = rast.shape[:2]
    pos = np.ascontiguousarray(pos, dtype=F32)
    tri = np.asarray(tri, dtype=np.int64)
    ok, X, Y, _, _ = snap_vertices(pos, H, W)
    V = pos.shape[0]
    wts = np.zeros((H, W, 4), dtype=F32)
    count = dict(to_outer=0, to_inner=0, horizontal=0, vertical=0, fold=0, boundary=0)
    ids = rast[..., 3].astype(np.int64)
    zs = rast[..., 2]
    steps = ((0, -1), (0, 1), (-1, 0), (1, 0))
    for r in range(H):
        for c in range(W):
            for k, (dr, dc) in enumerate(steps):
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
                t = (idp if inner else idn) - 1
                ri, ci = (r, c) if inner else (rn, cn)
                horizontal = dr == 0
                vi = tri[t]
                if not ok[vi].all():
                    continue
                L = 256 * r + 128 if horizontal else 256 * c + 128
                line = F32(r if horizontal else c) + F32(0.5)
                centre = F32(ci if horizontal else ri) + F32(0.5)
                for i in range(3):
                    a, b, cc, d = vi[(i + 1) % 3], vi[(i + 2) % 3], vi[i], int(opp[t, i])
                    kind = None
                    if d < 0 or d >= V or not ok[d]:
                        kind = "boundary"
                    else:
                        ex, ey = int(X[b] - X[a]), int(Y[b] - Y[a])
                        sc = ex * int(Y[cc] - Y[a]) - ey * int(X[cc] - X[a])
                        sd = ex * int(Y[d] - Y[a]) - ey * int(X[d] - X[a])
                        if sc * sd >= 0:                       # python integers: no overflow
                            kind = "fold"
                    if kind is None:
                        continue
                    a_on, b_on = (Y[a], Y[b]) if horizontal else (X[a], X[b])
                    a_al, b_al = (X[a], X[b]) if horizontal else (Y[a], Y[b])
                    if (a_on <= L) == (b_on <= L):
                        continue
                    sa_on, sb_on = F32(a_on) / F32(256), F32(b_on) / F32(256)
                    sa_al, sb_al = F32(a_al) / F32(256), F32(b_al) / F32(256)
                    x = sa_al + (sb_al - sa_al) * ((line - sa_on) / (sb_on - sa_on))
                    tt = np.abs(x - centre)
                    assert tt.dtype == F32
                    if not tt <= F32(1):
                        continue
                    wgt = F32(0)
                    if tt > F32(0.5):
                        if not inner:
                            wgt = tt - F32(0.5)
                            count["to_outer"] += 1
                    elif inner:
                        wgt = F32(0.5) - tt
                        count["to_inner"] += wgt != 0
                    if wgt != 0:
                        count["horizontal" if horizontal else "vertical"] += 1
                        count[kind] += 1
                    wts[r, c, k] = wgt
                    break
    if info is not None:
        info.update(count)
    return wts


def _neighbours(x):
    """The four neighbour images of x [H,W,C] (left, right, row - 1, row + 1); zero outside the frame."""
    z = np.zeros_like(x)
    left, right, up, down = z.copy(), z.copy(), z.copy(), z.copy()
    left[:, 1:], right[:, :-1] = x[:, :-1], x[:, 1:]
    up[1:], down[:-1] = x[:-1], x[1:]
    return left, right, up, down


def antialias_apply(x, wts):
    """out = in + sum_k w_k (in[n_k] - in), k in order, zero weights skipped (fp32)."""
    x = np.ascontiguousarray(x, dtype=F32)
    acc = x.copy()
    for k, nb in enumerate(_neighbours(x)):
        w = wts[..., k:k + 1]
        acc = np.where(w != 0, acc + w * (nb - x), acc)
    assert acc.dtype == F32
    return acc


def antialias_adjoint(y, wts):
    """din = dout (1 - sum_k w_k) + sum_k wts[n_k, opposite(k)] dout[n_k] (float64: the checker of the adjoint)."""
    y = y.astype(np.float64)
    w = wts.astype(np.float64)
    out = y * (1.0 - w.sum(axis=-1, keepdims=True))
    for k, ko in enumerate((1, 0, 3, 2)):
        out += _neighbours(w[..., ko:ko + 1])[k] * _neighbours(y)[k]
    return out
