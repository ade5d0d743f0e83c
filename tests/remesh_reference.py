"""The statement of the remesher of include/gd_mesh_remesh.h in numpy, written sequentially: the same passes, rounds and keys
as the kernels of csrc/raster_remesh.hip, in float64 or float32 (``dtype``), always from the float32 input the kernels see.

Every pass records in ``Margins`` the smallest relative margin by which a comparison it makes is decided: the length tests
against hi^2 and lo^2, the collapse guard, the split's diagonal choice, and the normal dot products (normalised by the two
lengths).  Where every margin is well above the fp32 rounding of those quantities, the float64 statement and the fp32
kernels decide alike and their discrete results are equal.

Nothing here is taken from a remeshing library; the test meshes are built below."""
import numpy as np

NORM_EPS = 1e-12
COLLAPSE_ROUNDS = 4


class Margins:
    """the smallest relative margin of each kind of comparison"""

    def __init__(self):
        self.smallest = {}

    def note(self, kind, values):
        values = np.atleast_1d(np.asarray(values, dtype=np.float64))
        if values.size:
            self.smallest[kind] = min(self.smallest.get(kind, np.inf), float(values.min()))

    def minimum(self):
        return min(self.smallest.values()) if self.smallest else np.inf


# ---- meshes -----------------------------------------------------------------------------------------------------------------

def cloth(n=10, seed=3, jitter=0.25):
    """An open patch of n x n quads over [0, 1]^2 with a sinusoidal height and seeded in-plane jitter of the inner vertices
    (a fraction of the spacing); float32 vertices, int64 triangles."""
    g = np.arange(n + 1) / n
    x, y = np.meshgrid(g, g, indexing="xy")
    rng = np.random.RandomState(seed)
    inner = ((x > 0) & (x < 1) & (y > 0) & (y < 1)).astype(np.float64)
    x = x + inner * rng.uniform(-jitter, jitter, x.shape) / n
    y = y + inner * rng.uniform(-jitter, jitter, y.shape) / n
    z = 0.1 * np.sin(2.5 * x + 0.5) * np.cos(2.0 * y + 0.3)          # no side of the patch is a straight line
    v = np.stack((x, y, z), axis=-1).reshape(-1, 3)
    idx = lambda i, j: j * (n + 1) + i
    tri = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            tri += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    return v.astype(np.float32), np.array(tri, dtype=np.int64)


def jittered_tube(nu=24, nv=12, seed=5, jitter=0.25, r=0.3, h=1.0):
    """An open tube around z, its inner rings jittered along the surface (angle and height); the two rims stay."""
    rng = np.random.RandomState(seed)
    ang = 2.0 * np.pi * np.arange(nu) / nu
    rows = []
    for j in range(nv + 1):
        free = 0.0 if j in (0, nv) else 1.0
        a = ang + free * rng.uniform(-jitter, jitter, nu) * (2.0 * np.pi / nu)
        z = h * j / nv + free * rng.uniform(-jitter, jitter, nu) * (h / nv)
        rows.append(np.stack((r * np.cos(a), r * np.sin(a), z), axis=1))
    v = np.concatenate(rows)
    tri = []
    for j in range(nv):
        for i in range(nu):
            a, b = j * nu + i, j * nu + (i + 1) % nu
            c, d = a + nu, b + nu
            tri += [(a, b, d), (a, d, c)]
    return v.astype(np.float32), np.array(tri, dtype=np.int64)


def sphere(levels=2, stretch=1.5, seed=7, jitter=0.0):
    """An octahedron subdivided ``levels`` times onto the unit sphere and stretched along z: closed, 8 4^levels faces"""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    tri = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.array(p, dtype=np.float64) for p in v]
    for _ in range(levels):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in tri:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tri = out
    v = np.array(v)
    if jitter:
        v = v + np.random.RandomState(seed).normal(0.0, jitter, v.shape)
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
    v = v * np.array([0.5, 0.5, 0.5 * stretch])
    return v.astype(np.float32), np.array(tri, dtype=np.int64)


SINGLE = (np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.3]]), np.array([[0, 1, 2]], dtype=np.int64))
QUAD = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [1.1, 1.0, 0.0], [0.0, 0.9, 0.2]]),
        np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64))          # mesh_geometry_reference.SINGLE / QUAD

# The seeds are pinned: on these meshes every comparison of a whole remesh (ten iterations, at every target the tests use)
# is decided by a relative margin of at least 1e-5 (test_mesh_remesh_cpu asserts it).
SEEDS = {"cloth": 3, "tube": 19, "sphere": 5}
MESHES = ["single", "quad", "cloth", "tube", "sphere", "cloth_extra"]
# What a GPU remesh may fall short of the float64 statement's quality: twice the largest difference between the float32
# and the float64 statement over the pinned cases (DESIGN.md 3.28 has the measured values).
QUALITY_MARGIN = {"share": 0.0, "valence": 0.0}


def mesh(name):
    """(float32 vertices, int64 triangles) of a test mesh by name"""
    if name == "single":
        return SINGLE[0].astype(np.float32), SINGLE[1]
    if name == "quad":
        return QUAD[0].astype(np.float32), QUAD[1]
    if name == "cloth":
        return cloth(10, seed=SEEDS["cloth"])
    if name == "tube":
        return jittered_tube(24, 12, seed=SEEDS["tube"])
    if name == "sphere":
        return sphere(2, 1.5, seed=SEEDS["sphere"], jitter=0.02)
    if name == "cloth_extra":
        v, tri = cloth(10, seed=SEEDS["cloth"])
        return np.concatenate((v[:7], np.array([[0.5, 0.5, 2.0]], dtype=np.float32), v[7:])), np.where(tri >= 7, tri + 1, tri)
    raise KeyError(name)


# ---- connectivity -----------------------------------------------------------------------------------------------------------

class Connectivity:
    def __init__(self, tri, V):
        tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
        F = tri.shape[0]
        if F and (tri.min() < 0 or tri.max() >= V):
            raise ValueError("vertex index out of range")
        if F and ((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0])).any():
            raise ValueError("a face lists a vertex twice")
        p, q = tri[:, [1, 2, 0]].ravel(), tri[:, [2, 0, 1]].ravel()          # half-edge k = 3 f + i
        key = (np.minimum(p, q) << 32) | np.maximum(p, q)
        order = np.argsort(key, kind="stable")
        sk = key[order]
        head = np.r_[True, sk[1:] != sk[:-1]] if F else np.zeros(0, bool)
        eid = np.cumsum(head) - 1
        count = np.bincount(eid) if F else np.zeros(0, np.int64)
        if F and count.max() > 2:
            raise ValueError("an edge is shared by more than two faces (non-manifold mesh)")
        start = np.flatnonzero(head)
        self.V, self.F, self.E = V, F, start.shape[0]
        self.tri = tri
        self.ev = np.stack((sk[start] >> 32, sk[start] & 0xffffffff), axis=1).reshape(-1, 2)
        self.eh = np.full((self.E, 2), -1, dtype=np.int64)
        self.eh[:, 0] = order[start]
        two = count == 2
        self.eh[two, 1] = order[start[two] + 1]
        self.fe = np.empty(3 * F, dtype=np.int64)
        self.fe[order] = eid
        self.bnd = np.zeros(V, dtype=bool)
        self.bnd[self.ev[~two].ravel()] = True
        src = np.concatenate((self.ev[:, 0], self.ev[:, 1]))
        dst = np.concatenate((self.ev[:, 1], self.ev[:, 0]))
        by = np.lexsort((dst, src))
        self.nbr_idx = dst[by]
        self.nbr_ptr = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(src, minlength=V), out=self.nbr_ptr[1:])
        corners = tri.ravel()
        self.vf_idx = np.argsort(corners, kind="stable")
        self.vf_ptr = np.zeros(V + 1, dtype=np.int64)
        np.cumsum(np.bincount(corners, minlength=V), out=self.vf_ptr[1:])

    def nbr(self, v):
        return self.nbr_idx[self.nbr_ptr[v]:self.nbr_ptr[v + 1]]

    def corners(self, v):
        return self.vf_idx[self.vf_ptr[v]:self.vf_ptr[v + 1]]

    def deg(self, v):
        return int(self.nbr_ptr[v + 1] - self.nbr_ptr[v])


# ---- arithmetic in the header's order -------------------------------------------------------------------------------------

def sqlen(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def cross(u, w):
    return np.stack((u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]), axis=-1)


def normal(p0, p1, p2):
    return cross(p1 - p0, p2 - p0)


def midpoint(p, q):
    return p.dtype.type(0.5) * (p + q)


def thresholds(h, dtype):
    """(lo^2, hi^2): the float32 values the kernels are given, in ``dtype``"""
    hi, lo = 4.0 / 3.0 * float(h), 4.0 / 5.0 * float(h)
    return dtype(np.float32(lo * lo)), dtype(np.float32(hi * hi))


def _dot_margin(margins, kind, d, n, m):
    """|cos| of the two normals.  Where one of them is EXACTLY zero (a boundary midpoint 0.5 (a + b) between a and b: the
    differences and products cancel exactly in either precision) the cosine is undefined and nothing is recorded: the dot
    product is an exact 0 in float64, in float32 and in the kernels alike, and `> 0` fails in all three."""
    scale = float(np.sqrt(dot(n, n)) * np.sqrt(dot(m, m)))
    if scale > 0.0:
        margins.note(kind, abs(float(d)) / scale)


# ---- split ------------------------------------------------------------------------------------------------------------------

def split(v, tri, h, margins=None):
    """(vertices, triangles, number of split edges)"""
    margins = margins or Margins()
    dt = v.dtype.type
    _, hi2 = thresholds(h, dt)
    c = Connectivity(tri, v.shape[0])
    if c.F == 0:
        return v.copy(), c.tri.copy(), 0
    len2 = sqlen(v[c.ev[:, 0]], v[c.ev[:, 1]])
    margins.note("split length", np.abs(len2 - hi2) / hi2)
    mark = len2 > hi2
    new = v.shape[0] + np.cumsum(mark) - mark
    mids = midpoint(v[c.ev[mark, 0]], v[c.ev[mark, 1]])
    out = []
    for f in range(c.F):
        t = [int(x) for x in c.tri[f]]
        m = [int(new[c.fe[3 * f + i]]) if mark[c.fe[3 * f + i]] else -1 for i in range(3)]
        nm = sum(x >= 0 for x in m)
        if nm == 0:
            out.append(tuple(t))
        elif nm == 1:
            i = [x >= 0 for x in m].index(True)
            a, b, cc = t[i], t[(i + 1) % 3], t[(i + 2) % 3]
            out += [(a, b, m[i]), (a, m[i], cc)]
        elif nm == 2:
            i = [x < 0 for x in m].index(True)
            a, b, cc = t[i], t[(i + 1) % 3], t[(i + 2) % 3]
            mca, mab = m[(i + 1) % 3], m[(i + 2) % 3]
            d_b = sqlen(v[b], midpoint(v[cc], v[a]))
            d_c = sqlen(midpoint(v[a], v[b]), v[cc])
            margins.note("split diagonal", abs(float(d_b) - float(d_c)) / max(float(d_b), float(d_c)))
            out.append((a, mab, mca))
            out += [(mab, b, mca), (b, cc, mca)] if d_b <= d_c else [(mab, b, cc), (mab, cc, mca)]
        else:
            out += [(t[0], m[2], m[1]), (t[1], m[0], m[2]), (t[2], m[1], m[0]), (m[0], m[1], m[2])]
    return np.concatenate((v, mids.astype(v.dtype))), np.array(out, dtype=np.int64).reshape(-1, 3), int(mark.sum())


# ---- collapse ---------------------------------------------------------------------------------------------------------------

def _collapse_allowed(c, v, a, b, interior, hi2, margins):
    if c.bnd[a] and interior:
        return False
    if c.bnd[a] and c.bnd[b] and interior:
        return False
    if np.intersect1d(c.nbr(a), c.nbr(b)).shape[0] != (2 if interior else 1):
        return False
    others = c.nbr(a)[c.nbr(a) != b]
    if others.shape[0]:
        d = sqlen(v[others], v[b])
        margins.note("collapse guard", np.abs(d - hi2) / hi2)
        if (d > hi2).any():
            return False
    for corner in c.corners(a):
        f, i = divmod(int(corner), 3)
        t = c.tri[f]
        if (t == b).any():
            continue
        p = [v[t[0]], v[t[1]], v[t[2]]]
        before = normal(*p)
        p[i] = v[b]
        after = normal(*p)
        d = dot(before, after)
        _dot_margin(margins, "collapse normals", d, before, after)
        if not d > 0:
            return False
    return True


def _length_key(len2, e):
    return (int(np.float32(len2).view(np.uint32)) << 32) | int(e)


def collapse_round(v, tri, h, margins=None):
    """(triangles with the dead faces removed in order, number of collapses); vertices keep their indices"""
    margins = margins or Margins()
    dt = v.dtype.type
    lo2, hi2 = thresholds(h, dt)
    c = Connectivity(tri, v.shape[0])
    if c.F == 0:
        return c.tri.copy(), 0
    len2 = sqlen(v[c.ev[:, 0]], v[c.ev[:, 1]])
    margins.note("collapse length", np.abs(len2 - lo2) / lo2)
    vkey = {}
    cand = {}
    for e in np.flatnonzero(len2 < lo2):
        lo, hi = int(c.ev[e, 0]), int(c.ev[e, 1])
        interior = c.eh[e, 1] >= 0
        if not interior and c.bnd[c.tri[c.eh[e, 0] // 3, c.eh[e, 0] % 3]]:
            continue                                                   # a face with all three vertices on the boundary stays
        if _collapse_allowed(c, v, lo, hi, interior, hi2, margins):
            a, b = lo, hi
        elif _collapse_allowed(c, v, hi, lo, interior, hi2, margins):
            a, b = hi, lo
        else:
            continue
        key = _length_key(len2[e], e)
        ring = {lo, hi} | set(c.nbr(lo).tolist()) | set(c.nbr(hi).tolist())
        cand[int(e)] = (a, b, key, ring)
        for x in ring:
            vkey[x] = min(vkey.get(x, key), key)
    remap = np.arange(v.shape[0])
    n = 0
    for e, (a, b, key, ring) in cand.items():
        if all(vkey[x] == key for x in ring):
            remap[a] = b
            n += 1
    t = remap[c.tri]
    alive = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])
    return t[alive], n


def compact_vertices(v, tri):
    """drop the vertices no face names, in order"""
    used = np.zeros(v.shape[0], dtype=bool)
    used[tri.ravel()] = True
    new = np.cumsum(used) - used
    return v[used], new[tri]


# ---- flip -------------------------------------------------------------------------------------------------------------------

def flip_round(v, tri, margins=None):
    """(triangles, number of flips)"""
    margins = margins or Margins()
    c = Connectivity(tri, v.shape[0])
    out = c.tri.copy()

    def cost(x, s):
        return abs(c.deg(x) + s - (4 if c.bnd[x] else 6))

    vkey, cand = {}, {}
    for e in np.flatnonzero(c.eh[:, 1] >= 0):
        (f0, i0), (f1, i1) = divmod(int(c.eh[e, 0]), 3), divmod(int(c.eh[e, 1]), 3)
        cc, p, q = (int(c.tri[f0, (i0 + s) % 3]) for s in range(3))
        d, p1, q1 = (int(c.tri[f1, (i1 + s) % 3]) for s in range(3))
        if f0 == f1 or p1 != q or q1 != p or cc == d or d in c.nbr(cc):
            continue
        before = cost(p, 0) + cost(q, 0) + cost(cc, 0) + cost(d, 0)
        after = cost(p, -1) + cost(q, -1) + cost(cc, 1) + cost(d, 1)
        if not after < before:
            continue
        n0, n1 = normal(v[cc], v[p], v[q]), normal(v[d], v[q], v[p])
        m0, m1 = normal(v[cc], v[p], v[d]), normal(v[cc], v[d], v[q])
        ok = True
        for m in (m0, m1):
            for n in (n0, n1):
                x = dot(m, n)
                _dot_margin(margins, "flip normals", x, m, n)
                ok = ok and bool(x > 0)
        if not ok:
            continue
        key = ((after - before + (1 << 30)) << 32) | int(e)
        cand[int(e)] = (cc, p, q, d, f0, f1, key)
        for x in (cc, p, q, d):
            vkey[x] = min(vkey.get(x, key), key)
    n = 0
    for e, (cc, p, q, d, f0, f1, key) in cand.items():
        if all(vkey[x] == key for x in (cc, p, q, d)):
            out[f0] = (cc, p, d)
            out[f1] = (cc, d, q)
            n += 1
    return out, n


# ---- relax ------------------------------------------------------------------------------------------------------------------

def relax(v, tri):
    """(vertices, moved mask): Jacobi, from the old positions"""
    c = Connectivity(tri, v.shape[0])
    dt = v.dtype.type
    out = v.copy()
    moved = np.zeros(v.shape[0], dtype=bool)
    for x in range(v.shape[0]):
        if c.bnd[x] or c.deg(x) == 0:
            continue
        s = np.zeros(3, dtype=v.dtype)
        for j in c.nbr(x):
            s = s + v[j]
        d = s / dt(c.deg(x)) - v[x]
        n = np.zeros(3, dtype=v.dtype)
        for corner in c.corners(x):
            t = c.tri[int(corner) // 3]
            n = n + normal(v[t[0]], v[t[1]], v[t[2]])
        n = n / max(np.sqrt(dot(n, n)), dt(NORM_EPS))
        t = dot(n, d)
        out[x] = v[x] + (d - n * t)
        moved[x] = True
    return out, moved


# ---- project ----------------------------------------------------------------------------------------------------------------

def closest_on_triangles(p, a, b, c):
    """closest point of each triangle (a, b, c) [M,3] to each p [N,3]: [N,M,3], the header's region tests"""
    p, a, b, c = p[:, None, :], a[None], b[None], c[None]
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = p - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (va + vb) + vc
        r = (a + ab * (vb / s)[..., None]) + ac * (vc / s)[..., None]
        on_bc = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        r = np.where(on_bc[..., None], b + (c - b) * ((d4 - d3) / ((d4 - d3) + (d5 - d6)))[..., None], r)
        on_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        r = np.where(on_ac[..., None], a + ac * (d2 / (d2 - d6))[..., None], r)
        r = np.where(((d6 >= 0) & (d5 <= d6))[..., None], c, r)
        on_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        r = np.where(on_ab[..., None], a + ab * (d1 / (d1 - d3))[..., None], r)
        r = np.where(((d3 >= 0) & (d4 <= d3))[..., None], b, r)
        r = np.where(((d1 <= 0) & (d2 <= 0))[..., None], a, r)
    return r


def closest_on_surface(p, sv, stri, chunk=256):
    """(closest points [N,3], squared distances [N]) of ``p`` on the surface (sv, stri), over ALL triangles; the lowest
    triangle index on a tie"""
    a, b, c = sv[stri[:, 0]], sv[stri[:, 1]], sv[stri[:, 2]]
    out, dist = np.empty_like(p), np.empty(p.shape[0], dtype=p.dtype)
    for i in range(0, p.shape[0], chunk):
        q = p[i:i + chunk]
        r = closest_on_triangles(q, a, b, c)
        d2 = sqlen(r, q[:, None, :])
        d2 = np.where(np.isnan(d2), np.inf, d2)
        best = np.argmin(d2, axis=1)                                  # the first minimum: the lowest index
        rows = np.arange(q.shape[0])
        out[i:i + chunk], dist[i:i + chunk] = r[rows, best], d2[rows, best]
    return out, dist


def cell_size(sv, stri, h):
    c = Connectivity(stri, sv.shape[0])
    longest = float(np.sqrt(sqlen(sv[c.ev[:, 0]], sv[c.ev[:, 1]]).max()))
    return max(longest, 4.0 / 3.0 * float(h))


def project(v, moved, sv, stri, cell):
    """(vertices, number left unprojected): the moved vertices go to their closest point if it is within ``cell``"""
    out = v.copy()
    idx = np.flatnonzero(moved)
    if idx.shape[0] == 0:
        return out, 0
    r, d2 = closest_on_surface(v[idx], sv, stri)
    near = d2 <= v.dtype.type(np.float32(cell)) ** 2
    out[idx[near]] = r[near]
    return out, int((~near).sum())


# ---- the whole remesh -------------------------------------------------------------------------------------------------------

def remesh(v32, tri, h, iterations=10, rounds=COLLAPSE_ROUNDS, dtype=np.float64, do_project=True, margins=None):
    """(vertices in ``dtype``, triangles int64, info, margins) from float32 vertices"""
    margins = margins or Margins()
    v = np.asarray(v32, dtype=np.float32).astype(dtype)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    Connectivity(tri, v.shape[0])                                      # the input's own errors
    v, tri = compact_vertices(v, tri)
    sv, stri = v.copy(), tri.copy()
    cell = cell_size(sv, stri, h) if tri.shape[0] else 1.0
    info = {"split": [], "collapsed": [], "flipped": [], "unprojected": [], "moved_most": 0.0, "longest_after_split": []}
    for _ in range(iterations):
        v, tri, n = split(v, tri, h, margins)
        info["split"].append(n)
        info["longest_after_split"].append(float(edge_lengths(v, tri).max()) / float(h) if tri.shape[0] else 0.0)
        total = 0
        for _ in range(rounds):
            tri, n = collapse_round(v, tri, h, margins)
            total += n
            if n == 0:
                break
        v, tri = compact_vertices(v, tri)
        info["collapsed"].append(total)
        total = 0
        for _ in range(rounds):
            tri, n = flip_round(v, tri, margins)
            total += n
            if n == 0:
                break
        info["flipped"].append(total)
        v, moved = relax(v, tri)
        n = 0
        if do_project:
            before = v
            v, n = project(v, moved, sv, stri, cell)
            info["moved_most"] = max(info["moved_most"], float(np.sqrt(sqlen(v, before).max())) / float(h))
        info["unprojected"].append(n)
    return v, tri, info, margins


def flip_test_mesh():
    """(float32 vertices, triangles) for one flip round: the cloth after one whole iteration at half its mean edge length
    and one more split, all in float32.  (The cloth with EVERY edge split has valences 4, 6 and 8 arranged so that no flip
    lowers the valence error: a round on it selects nothing.)"""
    v, tri = mesh("cloth")
    h = 0.5 * mean_edge_length(v, tri)
    v, tri, _, _ = remesh(v, tri, h, iterations=1, dtype=np.float32)
    v, tri, _ = split(v, tri, h)
    return v, tri


# ---- what the tests measure ---------------------------------------------------------------------------------------------------

def edge_lengths(v, tri):
    c = Connectivity(tri, v.shape[0])
    return np.sqrt(sqlen(v[c.ev[:, 0]].astype(np.float64), v[c.ev[:, 1]].astype(np.float64)))


def mean_edge_length(v, tri):
    return float(edge_lengths(v, tri).mean())


def boundary_loops(tri, V):
    """number of closed loops the boundary edges form"""
    c = Connectivity(tri, V)
    be = c.ev[c.eh[:, 1] < 0]
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in be.tolist():
        parent[find(a)] = find(b)
    return len({find(x) for x in list(parent)})


def invariants(v, tri):
    """The hard invariants of a remeshed surface, asserted; returns (Euler characteristic, boundary loops)."""
    tri = np.asarray(tri, dtype=np.int64)
    V = v.shape[0]
    assert np.isfinite(v).all()
    c = Connectivity(tri, V)                                           # raises on a repeated vertex or a third face on an edge
    assert np.unique(np.sort(tri, axis=1), axis=0).shape[0] == tri.shape[0], "duplicate faces"
    assert np.unique(tri).shape[0] == V, "an output vertex is referenced by no face"
    for e in np.flatnonzero(c.eh[:, 1] >= 0):                          # consistent orientation across interior edges
        (f0, i0), (f1, i1) = divmod(int(c.eh[e, 0]), 3), divmod(int(c.eh[e, 1]), 3)
        assert tri[f0, (i0 + 1) % 3] == tri[f1, (i1 + 2) % 3] and tri[f0, (i0 + 2) % 3] == tri[f1, (i1 + 1) % 3]
    return V - c.E + c.F, boundary_loops(tri, V)


def quality(v, tri, h):
    """(share of edges with length in [4/5 h, 4/3 h], mean |valence - target|)"""
    c = Connectivity(tri, v.shape[0])
    length = edge_lengths(v, tri)
    share = float(((length >= 0.8 * h) & (length <= 4.0 / 3.0 * h)).mean())
    deg = np.diff(c.nbr_ptr)
    return share, float(np.abs(deg - np.where(c.bnd, 4, 6)).mean())
