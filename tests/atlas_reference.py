"""numpy statement of the chart-based UV atlas (include/gd_atlas.h), steps 1-6: the checker of tests/test_texture_atlas_*.py.
Face classes in float32 in the header's order; charts by union-find; bounds through the order-preserving keys; a packer
of its own, in Python integers; corners on the 1/256-texel grid; coverage at texel centres by the rasterizer's rule
(include/gd_mesh.h, the rule of bake_reference.chart_coverage, here per face over its bounding box); the overlap peeling.
And the meshes of those tests.  Test infrastructure: never imported by the package."""
import functools

import numpy as np

from tests import mesh_scenes as scenes
from tests import remesh_reference as rr

DEGENERATE = 6
BISECTION_STEPS = 24
F32 = np.float32


# ---- meshes ---------------------------------------------------------------------------------------------------------------------

def cube(n=4):
    """closed axis-aligned cube [0, n]^3, n x n quads per side, outward normals, welded: 12 n^2 faces"""
    index, verts, tris = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for axis in range(3):
        for side in (0, 1):
            a1, a2 = (axis + 1) % 3, (axis + 2) % 3
            for i in range(n):
                for j in range(n):
                    def corner(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[a1], p[a2] = side * n, i + di, j + dj
                        return vid(tuple(p))
                    q = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]       # a1 x a2 = +axis
                    if side == 0:
                        q = q[::-1]
                    tris += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return np.array(verts, dtype=np.float32) / F32(n), np.array(tris, dtype=np.int32)


def helicoid(turns=1.5, r0=0.5, r1=1.0, nt=48, nr=4, pitch=0.05):
    """a strip around z: one component of class +z that lies over itself in projection for turns > 1; faces in the order
    of the angle, so the later sheet loses"""
    theta = 2.0 * np.pi * turns * np.arange(nt + 1) / nt
    rad = r0 + (r1 - r0) * np.arange(nr + 1) / nr
    v = np.array([[r * np.cos(t), r * np.sin(t), pitch * t] for t in theta for r in rad], dtype=np.float64)
    tris = []
    for i in range(nt):
        for j in range(nr):
            a, b, c, d = i * (nr + 1) + j, i * (nr + 1) + j + 1, (i + 1) * (nr + 1) + j + 1, (i + 1) * (nr + 1) + j
            tris += [[a, b, c], [a, c, d]]
    return v.astype(np.float32), np.array(tris, dtype=np.int32)


def strip(n=2048):
    """1 x n quads in the plane z = 0: the faces form a path"""
    v = np.array([[i * 0.01, j * 0.01, 0.0] for i in range(n + 1) for j in range(2)], dtype=np.float32)
    tris = []
    for i in range(n):
        a, b, c, d = 2 * i, 2 * i + 2, 2 * i + 3, 2 * i + 1
        tris += [[a, b, c], [a, c, d]]
    return v, np.array(tris, dtype=np.int32)


def two_squares():
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [3, 0, 1], [4, 0, 1], [4, 1, 1], [3, 1, 1]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=np.int32)


def ties():
    """faces whose normals are exactly (1, 1, 0), (-1, -1, 0), (0, 1, 1), (1, 0, 1) and (1, 1, 1): classes 0, 1, 2, 0, 0"""
    v = np.array([[0, 0, 0], [1, -1, 0], [0, 0, -1],          # u = (1, -1, 0), w = (0, 0, -1): n = (1, 1, 0)
                  [0, 0, 1],                                  # w = (0, 0, 1): n = (-1, -1, 0)
                  [1, 0, 0], [0, 1, -1],                      # u = (1, 0, 0), w = (0, 1, -1): n = (0, 1, 1)
                  [0, 1, 0], [1, 0, -1],                      # u = (0, 1, 0), w = (1, 0, -1): n = (-1, 0, -1) -> reversed
                  [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    tri = np.array([[0, 1, 2], [0, 1, 3], [0, 4, 5], [0, 7, 6], [4, 6, 3]], dtype=np.int32)
    return v, tri


def with_degenerate():
    """two squares and, between their faces, a face of three collinear vertices and one with a NaN vertex"""
    v, tri = two_squares()
    extra = np.array([[5, 5, 5], [6, 6, 6], [7, 7, 7], [8, 0, 0], [9, 0, 0], [np.nan, 1, 0]], dtype=np.float32)
    n = v.shape[0]
    tri = np.concatenate((tri[:2], [[n, n + 1, n + 2]], tri[2:], [[n + 3, n + 4, n + 5]])).astype(np.int32)
    return np.concatenate((v, extra)), tri


def single():
    return np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.25]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


def fan():
    """an edge shared by three faces"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int32)


def tube():
    v, tri, _ = scenes.tube(24, 12)
    return v, tri


# name -> (mesh, resolution, gutter) of the packed cases
PACKED = {"tube": (tube, 256, 2), "cube": (cube, 128, 2), "helicoid": (helicoid, 256, 2), "two_squares": (two_squares, 64, 2),
          "with_degenerate": (with_degenerate, 64, 1), "single": (single, 32, 2)}


# ---- 1. face class ----------------------------------------------------------------------------------------------------------------

def face_normals(v, tri):
    v = np.asarray(v, dtype=F32)
    p0, p1, p2 = (v[tri[:, i]] for i in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        u, w = p1 - p0, p2 - p0
        return np.stack((u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                         u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]), axis=1).astype(F32)


def face_class(v, tri):
    n = face_normals(v, tri)
    out = np.full(tri.shape[0], DEGENERATE, dtype=np.int32)
    for f in range(tri.shape[0]):
        if not np.isfinite(n[f]).all() or not n[f].any():
            continue
        k = 0
        for c in (1, 2):
            if abs(n[f, c]) > abs(n[f, k]):
                k = c
        out[f] = 2 * k + (1 if n[f, k] < 0 else 0)
    return out


def projected(v, tri, cls):
    """(a, b) float32 [F,3] of every corner; zeros for a degenerate face"""
    v = np.asarray(v, dtype=F32)
    a, b = np.zeros(tri.shape, dtype=F32), np.zeros(tri.shape, dtype=F32)
    for f in range(tri.shape[0]):
        if cls[f] == DEGENERATE:
            continue
        k = cls[f] // 2
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        if cls[f] % 2:
            k1, k2 = k2, k1
        a[f], b[f] = v[tri[f], k1], v[tri[f], k2]
    return a, b


# ---- 2. charts ----------------------------------------------------------------------------------------------------------------------

def chart_labels(conn, cls, layer=None, single_=None):
    """int32 [F]: the lowest face index of each face's component, by union-find"""
    F = conn.F
    layer = np.zeros(F, np.int32) if layer is None else layer
    single_ = np.zeros(F, np.int32) if single_ is None else single_
    parent = list(range(F))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for h0, h1 in conn.eh.tolist():
        if h1 < 0:
            continue
        f, g = h0 // 3, h1 // 3
        if cls[f] != cls[g] or cls[f] == DEGENERATE or layer[f] != layer[g] or single_[f] or single_[g]:
            continue
        rf, rg = find(f), find(g)
        if rf != rg:
            parent[max(rf, rg)] = min(rf, rg)
    return np.array([find(f) for f in range(F)], dtype=np.int32)


def face_charts(cls, labels):
    """(C, face_chart int32 [F]): charts numbered by ascending label; -1 for a degenerate face"""
    roots = np.array(sorted({int(x) for f, x in enumerate(labels) if cls[f] != DEGENERATE}), dtype=np.int64)
    number = {int(r): i for i, r in enumerate(roots)}
    return len(roots), np.array([number[int(x)] if cls[f] != DEGENERATE else -1 for f, x in enumerate(labels)], dtype=np.int32)


# ---- 3. bounds ----------------------------------------------------------------------------------------------------------------------

def order_key(x):
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    return np.where(u >> 31, u ^ 0xFFFFFFFF, u ^ 0x80000000).astype(np.uint32)


def order_value(k):
    k = np.asarray(k, dtype=np.uint32).astype(np.uint64)
    return np.where(k >> 31, k ^ 0x80000000, k ^ 0xFFFFFFFF).astype(np.uint32).view(F32)


def chart_bounds(a, b, face_chart, C):
    """(bounds float32 [C,4] = (a_min, b_min, a_max, b_max), count int32 [C])"""
    keys = np.empty((C, 4), dtype=np.uint32)
    keys[:, :2], keys[:, 2:] = 0xFFFFFFFF, 0
    count = np.zeros(C, dtype=np.int32)
    ka, kb = order_key(a), order_key(b)
    for f, c in enumerate(face_chart.tolist()):
        if c < 0:
            continue
        count[c] += 1
        keys[c, 0], keys[c, 1] = min(keys[c, 0], ka[f].min()), min(keys[c, 1], kb[f].min())
        keys[c, 2], keys[c, 3] = max(keys[c, 2], ka[f].max()), max(keys[c, 3], kb[f].max())
    return order_value(keys), count


# ---- 4. packing -----------------------------------------------------------------------------------------------------------------------

def rectangles(bounds, s, gutter):
    """Python integers [(w, h)] of the header's rectangles at the float32 scale ``s``"""
    s = F32(s)
    out = []
    for a0, b0, a1, b1 in np.asarray(bounds, dtype=F32):
        ma = int(np.rint(((a1 - a0) * s) * F32(256)))
        mb = int(np.rint(((b1 - b0) * s) * F32(256)))
        out.append((max((ma + 255) // 256, 1) + 2 * gutter, max((mb + 255) // 256, 1) + 2 * gutter))
    return out


def shelves(rects, resolution):
    """[(ox, oy)] per chart, or None"""
    order = sorted(range(len(rects)), key=lambda c: (-rects[c][1], -rects[c][0], c))
    out = [None] * len(rects)
    x = y = shelf = 0
    fresh = True
    for c in order:
        w, h = rects[c]
        if w > resolution:
            return None
        if x + w > resolution:
            y, x, fresh = y + shelf, 0, True
        if fresh:
            shelf, fresh = h, False
        if y + h > resolution:
            return None
        out[c] = (x, y)
        x += w
    return out


def pack(bounds, resolution, gutter):
    """(scale float32, offsets [(ox, oy)], rectangles [(w, h)])"""
    def fit(s):
        rects = rectangles(bounds, s, gutter)
        off = shelves(rects, resolution)
        return None if off is None else (F32(s), off, rects)

    if fit(0.0) is None:
        raise ValueError("the resolution is too small for the gutters of the charts")
    d = np.asarray(bounds, dtype=np.float64)
    d = float(max((d[:, 2] - d[:, 0]).max(), (d[:, 3] - d[:, 1]).max()))
    hi = (resolution - 2 * gutter) / d
    best = fit(F32(hi))
    if best is not None:
        return best
    lo = 0.0
    for _ in range(BISECTION_STEPS):
        mid = float(F32((lo + hi) / 2))
        got = fit(mid)
        if got is not None:
            lo, best = mid, got
        else:
            hi = mid
    if best is None or not best[0] > 0:
        raise ValueError("the resolution is too small for the gutters of the charts")
    return best


# ---- 5. corners -----------------------------------------------------------------------------------------------------------------------

def emit(a, b, tri, face_chart, bounds, C, offsets, s, gutter, resolution):
    """(corner_xy int32 [F,3,2], vt float32 [T,2], ft int32 [F,3])"""
    F = tri.shape[0]
    s = F32(s)
    xy = np.zeros((F, 3, 2), dtype=np.int32)
    key = np.full((F, 3), C << 32, dtype=np.int64)
    for f, c in enumerate(face_chart.tolist()):
        if c < 0:
            continue
        xy[f, :, 0] = 256 * (offsets[c][0] + gutter) + np.rint(((a[f] - bounds[c, 0]) * s) * F32(256)).astype(np.int32)
        xy[f, :, 1] = 256 * (offsets[c][1] + gutter) + np.rint(((b[f] - bounds[c, 1]) * s) * F32(256)).astype(np.int32)
        key[f] = (c << 32) | tri[f].astype(np.int64)
    rows, first, inverse = np.unique(key.ravel(), return_index=True, return_inverse=True)
    vt = xy.reshape(-1, 2)[first].astype(F32) / F32(256 * resolution)
    assert np.array_equal(xy.reshape(-1, 2)[first][inverse.ravel()], xy.reshape(-1, 2))     # a row has one position
    return xy, vt.astype(F32), inverse.reshape(F, 3).astype(np.int32)


# ---- 6. coverage and lost faces -----------------------------------------------------------------------------------------------------------

def face_cover(xy, H, W):
    """(rows, cols) of the texel centres the triangle with corners ``xy`` int [3,2] (1/256 texel) covers, by the rule of
    include/gd_mesh.h as bake_reference.chart_coverage has it"""
    x, y = [int(t) for t in xy[:, 0]], [int(t) for t in xy[:, 1]]
    A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    if A == 0:
        return none
    c0, c1 = max(0, -((128 - min(x)) // 256)), min(W - 1, (max(x) - 128) // 256)
    r0, r1 = max(0, -((128 - min(y)) // 256)), min(H - 1, (max(y) - 128) // 256)
    if c1 < c0 or r1 < r0:
        return none
    Px = (256 * np.arange(c0, c1 + 1, dtype=np.int64) + 128)[None, :]
    Py = (256 * np.arange(r0, r1 + 1, dtype=np.int64) + 128)[:, None]
    sign = 1 if A > 0 else -1
    inside = np.ones((r1 - r0 + 1, c1 - c0 + 1), dtype=bool)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        dX, dY = sign * (x[k] - x[j]), sign * (y[k] - y[j])
        e = dX * (Py - y[j]) - dY * (Px - x[j])
        inside &= (e > 0) | ((e == 0) & ((dY > 0) or (dY == 0 and dX < 0)))
    r, c = np.nonzero(inside)
    return r + r0, c + c0


def owners(xy, H, W):
    """(owner int32 [H,W]: the lowest face that covers each centre, -1 for none; times int32 [H,W]: how many cover it)"""
    owner = np.full((H, W), -1, dtype=np.int32)
    times = np.zeros((H, W), dtype=np.int32)
    for f in range(xy.shape[0] - 1, -1, -1):
        r, c = face_cover(xy[f], H, W)
        owner[r, c] = f
        times[r, c] += 1
    return owner, times


def lost_faces(xy, owner):
    H, W = owner.shape
    lost = np.zeros(xy.shape[0], dtype=np.int32)
    for f in range(xy.shape[0]):
        r, c = face_cover(xy[f], H, W)
        lost[f] = int((owner[r, c] != f).any())
    return lost


# ---- the whole ------------------------------------------------------------------------------------------------------------------------------

def chart_atlas(v, tri, resolution, gutter=2, max_rounds=8):
    """dict: ``vt``, ``ft``, ``face_chart``, ``num_charts``, ``scale``, ``rounds``, ``lost_per_round``, ``singletons``,
    ``seam_edges``, ``coverage``, ``owner``, ``times``, ``offsets``, ``rects``, ``cls``, ``corner_xy`` and ``trace``, one
    dict per round with what the round started from and made"""
    v, tri = np.asarray(v, dtype=F32), np.asarray(tri, dtype=np.int32)
    F = tri.shape[0]
    conn = rr.Connectivity(tri, v.shape[0])
    cls = face_class(v, tri)
    a, b = projected(v, tri, cls)
    layer, single_ = np.zeros(F, np.int32), np.zeros(F, np.int32)
    trace = []
    while True:
        rnd = len(trace) + 1
        labels = chart_labels(conn, cls, layer, single_)
        C, face_chart = face_charts(cls, labels)
        if C == 0:
            raise ValueError("every face is degenerate")
        bounds, count = chart_bounds(a, b, face_chart, C)
        s, offsets, rects = pack(bounds, resolution, gutter)
        xy, vt, ft = emit(a, b, tri, face_chart, bounds, C, offsets, s, gutter, resolution)
        owner, times = owners(xy, resolution, resolution)
        lost = lost_faces(xy, owner)
        trace.append(dict(layer=layer.copy(), single=single_.copy(), labels=labels, face_chart=face_chart, bounds=bounds,
                          count=count, scale=s, offsets=np.array(offsets, np.int32), sizes=np.array(rects, np.int32),
                          corner_xy=xy, vt=vt, ft=ft, lost=lost))
        if not lost.any():
            break
        if rnd >= max_rounds:
            single_ = single_ | lost
        else:
            layer = layer + lost
        assert rnd < max_rounds + F
    fa, fb = face_chart[conn.eh[:, 0] // 3], face_chart[np.maximum(conn.eh[:, 1], 0) // 3]
    return dict(vt=vt, ft=ft, face_chart=face_chart, num_charts=C, scale=float(s), rounds=len(trace),
                lost_per_round=[int(t["lost"].sum()) for t in trace], singletons=int(single_.sum()),
                seam_edges=int(((conn.eh[:, 1] >= 0) & (fa != fb)).sum()), coverage=float((owner >= 0).sum()) / resolution ** 2,
                owner=owner, times=times, offsets=offsets, rects=rects, cls=cls, corner_xy=xy, trace=trace)


@functools.lru_cache(maxsize=None)
def packed(name):
    """the statement's atlas of a PACKED case: computed once, shared, read-only"""
    make, res, gutter = PACKED[name]
    v, tri = make()
    return v, tri, res, gutter, chart_atlas(v, tri, res, gutter)
