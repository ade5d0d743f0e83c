"""The statement of include/gd_mesh_simplify.h in numpy, written sequentially: quadric decimation by half-edge collapses (the
same rounds, passes and keys as the kernels of csrc/raster_simplify.hip), Taubin smoothing, the rotation of the final mesh.

Decimation is float64 from the float32 positions the kernels see; Taubin runs in float32 or float64 (``dtype``).  Every sum
is written out add by add in the header's order: no ``np.sum``, no ``@``, no ``einsum``, which reassociate or fuse.

The meshes, ``Connectivity``, ``invariants`` and ``closest_on_surface`` are those of tests/remesh_reference.py."""
import numpy as np

from tests.remesh_reference import (Connectivity, boundary_loops, cloth, closest_on_surface, compact_vertices,  # noqa: F401
                                    invariants, mesh as remesh_mesh, sphere)

NO_KEY = (1 << 63) - 1
PASSES = 4
MAX_ROUNDS = 1024
MESHES = ["single", "quad", "cloth", "tube", "sphere", "cloth_extra", "tetrahedron", "octahedron", "integer", "folded"]


# ---- meshes -----------------------------------------------------------------------------------------------------------------

def tetrahedron():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [0.1, 1.0, 0.0], [0.2, 0.3, 1.0]], dtype=np.float32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], dtype=np.int64)


def integer_mesh():
    """the 6 x 6 grid with integer x, y and integer heights in [0, 4]: every quadric and cost is an integer below 2^53.
    No face is degenerate: its x, y projection already has area 1/2."""
    n = 6
    g = np.arange(n + 1)
    x, y = np.meshgrid(g, g, indexing="xy")
    z = (3 * x + 5 * y + x * y) % 5
    v = np.stack((x, y, z), axis=-1).reshape(-1, 3).astype(np.float32)
    _, tri = cloth(n, seed=0, jitter=0.0)
    return v, tri


def folded_sheet():
    """cloth(12, seed=1) with z = max(x - 0.5, 0) + 0.02 sin(7 y + 3 x): a flat half, a crease and a ramp"""
    v, tri = cloth(12, seed=1)
    v = v.astype(np.float64)
    v[:, 2] = np.maximum(v[:, 0] - 0.5, 0.0) + 0.02 * np.sin(7.0 * v[:, 1] + 3.0 * v[:, 0])
    return v.astype(np.float32), tri


def mesh(name):
    """(float32 vertices, int64 triangles) of a test mesh by name"""
    if name == "tetrahedron":
        return tetrahedron()
    if name == "octahedron":
        return sphere(0)
    if name == "integer":
        return integer_mesh()
    if name == "folded":
        return folded_sheet()
    return remesh_mesh(name)


# ---- quadrics, in the header's order ------------------------------------------------------------------------------------------

def face_quadric(p0, p1, p2):
    """the ten entries (xx, xy, xz, xd, yy, yz, yd, zz, zd, dd) of [N; d][N; d]^T, float64"""
    u, w = p1 - p0, p2 - p0
    n0 = u[1] * w[2] - u[2] * w[1]
    n1 = u[2] * w[0] - u[0] * w[2]
    n2 = u[0] * w[1] - u[1] * w[0]
    d = -((n0 * p0[0] + n1 * p0[1]) + n2 * p0[2])
    return np.array([n0 * n0, n0 * n1, n0 * n2, n0 * d, n1 * n1, n1 * n2, n1 * d, n2 * n2, n2 * d, d * d], dtype=np.float64)


def vertex_quadrics(v32, c):
    """[V,10] float64: the sum of the face quadrics over the corners of each vertex, ascending, from 0"""
    p = np.asarray(v32, dtype=np.float32).astype(np.float64)
    q = np.zeros((c.V, 10), dtype=np.float64)
    for x in range(c.V):
        for corner in c.corners(x):
            t = c.tri[int(corner) // 3]
            q[x] = q[x] + face_quadric(p[t[0]], p[t[1]], p[t[2]])
    return q


def quadric_terms(q, p):
    """the ten terms whose ordered sum is the value of q at p"""
    x, y, z = p
    return [(q[0] * x) * x, (q[4] * y) * y, (q[7] * z) * z, (q[1] * x) * y, (q[2] * x) * z, (q[5] * y) * z,
            q[3] * x, q[6] * y, q[8] * z, q[9]]


def quadric_value(q, p):
    t = quadric_terms(q, p)
    squares = (t[0] + t[1]) + t[2]
    mixed = (t[3] + t[4]) + t[5]
    linear = (t[6] + t[7]) + t[8]
    return ((squares + 2.0 * mixed) + 2.0 * linear) + t[9]


def collapse_cost(q, p, a, b):
    """remove a, keep b where it is: (Q_a + Q_b)(p_b), clamped at 0"""
    value = quadric_value(q[a] + q[b], p[b])
    return value if value > 0.0 else 0.0


def _dot(p, q):
    return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]


def _normal(p0, p1, p2):
    u, w = p1 - p0, p2 - p0
    return np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]])


def allowed(c, p, a, b):
    """may a be removed onto b? (an interior edge)"""
    if c.bnd[a]:
        return False
    common = np.intersect1d(c.nbr(a), c.nbr(b))
    if common.shape[0] != 2:
        return False
    for n in common:
        if not c.deg(int(n)) > (2 if c.bnd[n] else 3):
            return False
    for corner in c.corners(a):
        f, i = divmod(int(corner), 3)
        t = c.tri[f]
        if (t == b).any():
            continue
        q = [p[t[0]], p[t[1]], p[t[2]]]
        before = _normal(*q)
        q[i] = p[b]
        if not _dot(before, _normal(*q)) > 0.0:
            return False
    return True


def key_of(cost, e):
    return (int(np.float32(cost).view(np.uint32)) << 32) | int(e)


def candidates(c, p, q, cost="quadric"):
    """(key int64-valued list [E], direction [E]: 0 none, 1 remove lo, 2 remove hi, costs [E,2] of lo -> hi and hi -> lo)"""
    keys, direction, costs = [NO_KEY] * c.E, [0] * c.E, np.zeros((c.E, 2))
    for e in range(c.E):
        lo, hi = int(c.ev[e, 0]), int(c.ev[e, 1])
        if cost == "quadric":
            costs[e] = collapse_cost(q, p, lo, hi), collapse_cost(q, p, hi, lo)
        else:
            d = p[lo] - p[hi]
            costs[e] = _dot(d, d)
        if c.eh[e, 1] < 0:
            continue
        order = (1, 2) if costs[e, 0] <= costs[e, 1] else (2, 1)
        for d in order:
            a, b = (lo, hi) if d == 1 else (hi, lo)
            if allowed(c, p, a, b):
                direction[e] = d
                keys[e] = key_of(costs[e, d - 1], e)
                break
    return keys, direction, costs


def decimation_round(p, tri, q, target, passes=PASSES, cost="quadric", trace=None):
    """One round on the connectivity of ``tri``: (triangles with the dead faces removed in order, selected); ``q`` is
    updated in place.  ``trace``, a dict, receives the keys, directions, costs, threshold and the winners of each pass."""
    c = Connectivity(tri, p.shape[0])
    keys, direction, costs = candidates(c, p, q, cost)
    m = -((target - c.F) // 2)                                          # ceil((F - target) / 2)
    threshold = sorted(keys)[min(m, c.E) - 1]
    live = [e for e in range(c.E) if keys[e] != NO_KEY and keys[e] <= threshold]
    ring = {e: set(c.ev[e].tolist()) | set(c.nbr(c.ev[e, 0]).tolist()) | set(c.nbr(c.ev[e, 1]).tolist()) for e in live}
    locked = np.zeros(c.V, dtype=bool)
    remap = np.arange(c.V)
    winners = []
    for _ in range(passes):
        vkey = {}
        for e in live:
            if not any(locked[x] for x in ring[e]):
                for x in ring[e]:
                    vkey[x] = min(vkey.get(x, keys[e]), keys[e])
        won = [e for e in live if all(vkey.get(x) == keys[e] for x in ring[e])]
        for e in won:
            lo, hi = int(c.ev[e, 0]), int(c.ev[e, 1])
            a, b = (lo, hi) if direction[e] == 1 else (hi, lo)
            remap[a] = b
            q[b] = q[b] + q[a]
            locked[list(ring[e])] = True
        winners.append(won)
    if trace is not None:
        trace.update(keys=keys, direction=direction, costs=costs, threshold=threshold, winners=winners, live=live)
    t = remap[c.tri]
    alive = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])
    return t[alive], sum(len(w) for w in winners)


def decimate(v32, tri, target, passes=PASSES, max_rounds=MAX_ROUNDS, cost="quadric"):
    """(float32 vertices, int64 triangles, info) of the decimation to ``target`` faces"""
    v32 = np.asarray(v32, dtype=np.float32)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    if target < 0:
        raise ValueError("target_faces must be >= 0")
    if passes < 1:
        raise ValueError("passes must be >= 1")
    info = {"reached": True, "selected": [], "faces": []}
    c = Connectivity(tri, v32.shape[0])                                 # the input's own errors
    if tri.shape[0] <= target:
        return v32.copy(), tri.copy(), info
    p = v32.astype(np.float64)
    q = vertex_quadrics(v32, c)
    while tri.shape[0] > target:
        if len(info["selected"]) >= max_rounds:
            info["reached"] = False
            break
        tri, n = decimation_round(p, tri, q, target, passes, cost)
        info["selected"].append(n)
        info["faces"].append(int(tri.shape[0]))
        if n == 0:
            info["reached"] = False
            break
    v, tri = compact_vertices(v32, tri)
    return v, tri, info


# ---- Taubin smoothing -----------------------------------------------------------------------------------------------------

def smooth_pass(v, c, w):
    """Jacobi: p + w (mean - p); an interior vertex averages its neighbours, a boundary vertex those it is joined to by a
    boundary edge, ascending; a vertex with none stays"""
    dt = v.dtype.type
    boundary = {(int(a), int(b)) for (a, b), h in zip(c.ev, c.eh) if h[1] < 0}
    out = v.copy()
    for x in range(c.V):
        s, k = np.zeros(3, dtype=v.dtype), 0
        for n in c.nbr(x):
            n = int(n)
            if c.bnd[x] and (min(x, n), max(x, n)) not in boundary:
                continue
            s = s + v[n]
            k += 1
        if k:
            out[x] = v[x] + dt(w) * (s / dt(k) - v[x])
    return out


def taubin(v32, tri, steps=10, lam=0.5, mu=-0.53, dtype=np.float64):
    """``steps`` x (a lam pass, a mu pass); the weights are the float32 values the kernels are given"""
    v = np.asarray(v32, dtype=np.float32).astype(dtype)
    c = Connectivity(tri, v.shape[0])
    for _ in range(steps):
        v = smooth_pass(v, c, np.float32(lam))
        v = smooth_pass(v, c, np.float32(mu))
    return v


# ---- the final mesh ---------------------------------------------------------------------------------------------------------

def rotate(v):
    """-90 degrees about x, exactly: (x, y, z) -> (x, z, -y)"""
    return np.stack((v[:, 0], v[:, 2], -v[:, 1]), axis=1)


def post_process(v32, tri, target=40000, smooth=True, do_rotate=True, dtype=np.float64):
    v = np.asarray(v32, dtype=np.float32)
    if do_rotate:
        v = rotate(v)
    v, tri, info = decimate(v, tri, target)
    if smooth and tri.shape[0]:
        v = taubin(v, tri, dtype=dtype)
    return v, tri, info


# ---- what the tests measure ---------------------------------------------------------------------------------------------------

def boundary_of(v, tri):
    """(set of boundary vertex positions as bytes, set of boundary edges as pairs of positions)"""
    c = Connectivity(tri, v.shape[0])
    pos = lambda x: np.asarray(v[x], dtype=np.float32).tobytes()
    edges = {frozenset((pos(a), pos(b))) for (a, b), h in zip(c.ev, c.eh) if h[1] < 0}
    return {pos(x) for x in np.flatnonzero(c.bnd)}, edges
