"""The statement of include/gd_mesh_clean.h in numpy, written sequentially: the literal sequential merge, components by
breadth-first search, the edge repair round by round, fans by flood fill.  Every fp32 operation is one numpy float32
operation, in the header's order: no ``np.sum``, no ``@``, which reassociate or fuse.

Nothing here is taken from a mesh library; the junk the tests add to the meshes of tests/remesh_reference.py is built
below."""
import math
from collections import deque

import numpy as np

f32 = np.float32
REPORT_KEYS = ("unreferenced", "merged", "merge_rounds", "null_faces", "duplicate_faces", "components", "components_removed",
               "component_faces_removed", "edge_faces_removed", "edge_rounds", "vertices_split")


# ---- sections 0 and 1 -------------------------------------------------------------------------------------------------------

def check(v, tri):
    """the referenced mask; the argument errors of the header"""
    v, tri = np.asarray(v), np.asarray(tri)
    if tri.size and (tri.min() < 0 or tri.max() >= v.shape[0]):
        raise ValueError("vertex index out of range")
    used = np.zeros(v.shape[0], dtype=bool)
    used[tri.reshape(-1)] = True
    if not np.isfinite(v[used]).all():
        raise ValueError("a position is not finite on a vertex some face references")
    return used


def diagonal(v, used):
    """D: float64, from the exact fp32 box of the referenced vertices"""
    p = v[used]
    lo, hi = p.min(axis=0), p.max(axis=0)
    d = [float(hi[a]) - float(lo[a]) for a in range(3)]
    return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def fraction(D, pct):
    return f32(D * float(pct) / 100.0)


def sq3(x, y, z):
    """fl(fl(fl(x x) + fl(y y)) + fl(z z)) on float32 scalars or arrays"""
    return (x * x + y * y) + z * z


def close_to(v, a, r2):
    """the mask of the vertices close to vertex a"""
    d = v - v[a]
    return sq3(d[:, 0], d[:, 1], d[:, 2]) <= r2


# ---- section 2 --------------------------------------------------------------------------------------------------------------

def merge_targets(v, used, r):
    """the literal sequential statement: target [V], -1 for a vertex no face names"""
    v = np.asarray(v, dtype=f32)
    r2 = f32(r) * f32(r)
    target = np.full(v.shape[0], -1, dtype=np.int64)
    for a in np.flatnonzero(used):
        if target[a] >= 0:
            continue
        near = close_to(v, a, r2) & used & (target < 0)
        target[near] = a                                                # a itself is among them: its distance is 0
    return target


def merge_rounds(v, used, r):
    """The Jacobi rounds of the header: (target, rounds).  The closeness graph is held as lists, so small inputs only."""
    v = np.asarray(v, dtype=f32)
    r2 = f32(r) * f32(r)
    ids = np.flatnonzero(used)
    lower = {int(a): [int(b) for b in np.flatnonzero(close_to(v, a, r2) & used) if b < a] for a in ids}
    state = {int(a): 0 for a in ids}
    rounds = 0
    while any(s == 0 for s in state.values()):
        new = dict(state)
        for a in ids:
            a = int(a)
            if state[a]:
                continue
            if any(state[b] == 1 for b in lower[a]):
                new[a] = 2
            elif all(state[b] == 2 for b in lower[a]):
                new[a] = 1
        state = new
        rounds += 1
    target = np.full(v.shape[0], -1, dtype=np.int64)
    for a in ids:
        a = int(a)
        target[a] = a if state[a] == 1 else min(b for b in lower[a] if state[b] == 1)
    return target, rounds


# ---- section 3 --------------------------------------------------------------------------------------------------------------

def face_normals(v, tri):
    v = np.asarray(v, dtype=f32)
    p0, p1, p2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    u, w = p1 - p0, p2 - p0
    return np.stack((u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                     u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]), axis=1)


def distinct(tri):
    return (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 0])


def null_faces(v, tri):
    """(alive bool [F], akey float32 [F])"""
    with np.errstate(all="ignore"):
        n = face_normals(v, tri)
        alive = distinct(tri) & np.isfinite(n).all(axis=1) & (n != 0).any(axis=1)
        akey = np.where(alive, sq3(n[:, 0], n[:, 1], n[:, 2]), f32(0)).astype(f32)
    return alive, akey


# ---- section 4 --------------------------------------------------------------------------------------------------------------

def in_table(tri, alive):
    return np.asarray(alive, dtype=bool) & distinct(tri)


def duplicate_faces(tri, alive):
    """bool [F]: every face of the table but the lowest of its unordered triple"""
    seen, dup = set(), np.zeros(tri.shape[0], dtype=bool)
    for f in np.flatnonzero(in_table(tri, alive)):
        key = tuple(sorted(tri[f].tolist()))
        dup[f] = key in seen
        seen.add(key)
    return dup


def edge_faces(tri, live):
    """{(lo, hi): faces in ascending order} over the faces of the table"""
    edges = {}
    for f in np.flatnonzero(live):
        a, b, c = tri[f].tolist()
        for p, q in ((b, c), (c, a), (a, b)):
            edges.setdefault((min(p, q), max(p, q)), []).append(int(f))
    return edges


# ---- section 5 --------------------------------------------------------------------------------------------------------------

def components(tri, alive):
    """label [F] by breadth-first search over shared edges: the lowest face index of the component, -1 for a dead face"""
    alive = np.asarray(alive, dtype=bool)
    live = in_table(tri, alive)
    edges = edge_faces(tri, live)
    label = np.full(tri.shape[0], -1, dtype=np.int64)
    for f in np.flatnonzero(alive):
        if label[f] >= 0:
            continue
        label[f] = f
        queue = deque([int(f)])
        while queue and live[f]:
            g = queue.popleft()
            a, b, c = tri[g].tolist()
            for p, q in ((b, c), (c, a), (a, b)):
                for h in edges[(min(p, q), max(p, q))]:
                    if label[h] < 0:
                        label[h] = f
                        queue.append(h)
    return label


def small_components(v, tri, alive, label, D, min_faces, min_diameter_pct):
    """(removed bool [F], components, components removed)"""
    v = np.asarray(v, dtype=f32)
    t = fraction(D, min_diameter_pct) if min_diameter_pct > 0 else f32(0)
    t2 = t * t
    removed = np.zeros(tri.shape[0], dtype=bool)
    roots = np.unique(label[label >= 0])
    gone = 0
    for root in roots:
        faces = np.flatnonzero(label == root)
        p = v[tri[faces].reshape(-1)]
        e = p.max(axis=0) - p.min(axis=0)
        if (min_faces > 0 and faces.size < min_faces) or (t2 > 0 and sq3(e[0], e[1], e[2]) < t2):
            removed[faces] = True
            gone += 1
    return removed, int(roots.size), gone


# ---- section 6 --------------------------------------------------------------------------------------------------------------

def edge_rounds(tri, alive, akey):
    """(alive', rounds): sequential rounds on the table of `alive`"""
    live = in_table(tri, alive)
    edges = edge_faces(tri, live)
    alive = np.asarray(alive, dtype=bool).copy()
    rounds = 0
    while True:
        nominated = []
        for faces in edges.values():
            now = [f for f in faces if alive[f]]
            if len(now) > 2:
                nominated.append(min(now, key=lambda f: (akey[f], -f)))
        if not nominated:
            return alive, rounds
        alive[nominated] = False
        rounds += 1


def one_shot_edge_rule(tri, alive, akey):
    """NOT the header's rule, for contrast in the tests: every edge with more than two faces keeps its two largest (the
    lowest index among equal keys) at once"""
    alive = np.asarray(alive, dtype=bool).copy()
    dead = set()
    for faces in edge_faces(tri, in_table(tri, alive)).values():
        if len(faces) > 2:
            dead.update(sorted(faces, key=lambda f: (akey[f], -f))[:-2])
    alive[sorted(dead)] = False
    return alive


def in_place_edge_round(tri, alive, akey):
    """NOT the header's rule either: one round in which the edges, in ascending (lo, hi), see the faces earlier edges of the
    same round have already removed"""
    alive = np.asarray(alive, dtype=bool).copy()
    edges = edge_faces(tri, in_table(tri, alive))
    for key in sorted(edges):
        now = [f for f in edges[key] if alive[f]]
        if len(now) > 2:
            alive[min(now, key=lambda f: (akey[f], -f))] = False
    return alive


# ---- section 7 --------------------------------------------------------------------------------------------------------------

def fans(tri, alive):
    """root [3F]: the lowest corner index of the fan of each corner of a live face by flood fill, -1 elsewhere"""
    live = in_table(tri, alive)
    edges = edge_faces(tri, live)
    root = np.full(3 * tri.shape[0], -1, dtype=np.int64)
    for c in range(3 * tri.shape[0]):
        f, v = c // 3, tri[c // 3, c % 3]
        if not alive[f] or root[c] >= 0:
            continue
        root[c] = c
        queue = deque([f])
        while queue and live[f]:
            g = queue.popleft()
            for x in tri[g].tolist():
                if x == v:
                    continue
                for h in edges[(min(x, v), max(x, v))]:                 # the faces across an edge incident to v
                    ch = 3 * h + tri[h].tolist().index(v)
                    if root[ch] < 0:
                        root[ch] = c
                        queue.append(h)
    return root


# ---- section 8 and the whole chain --------------------------------------------------------------------------------------------

def emit(v, tri, alive, target, root):
    """(vertices, indices, vertex_map, face_map, copies); `root` None: nothing is split"""
    v = np.asarray(v, dtype=f32)
    V = v.shape[0]
    face_map = np.flatnonzero(alive)
    used = np.zeros(V, dtype=bool)
    used[tri[face_map].reshape(-1)] = True
    row = np.cumsum(used) - 1
    V0 = int(used.sum())
    out = row[tri[face_map]]
    copies = []
    if root is not None and face_map.size:
        corners = (3 * face_map[:, None] + np.arange(3)[None, :]).reshape(-1)
        lowest = {}
        for c in corners:
            x = int(tri[c // 3, c % 3])
            lowest[x] = min(lowest.get(x, c), c)
        copies = sorted({(int(tri[root[c] // 3, root[c] % 3]), int(root[c])) for c in corners
                         if root[c] != lowest[int(tri[c // 3, c % 3])]})
        rank = {r: k for k, (_, r) in enumerate(copies)}
        for k, c in enumerate(corners):
            if int(root[c]) in rank:
                out[k // 3, k % 3] = V0 + rank[int(root[c])]
    vertices = np.concatenate((v[used], v[[x for x, _ in copies]].reshape(-1, 3))).astype(f32)
    vertex_map = np.full(V, -1, dtype=np.int64)
    has = target >= 0
    vertex_map[has] = np.where(used[target[has]], row[target[has]], -1)
    return vertices, out.reshape(-1, 3).astype(np.int64), vertex_map, face_map.astype(np.int64), len(copies)


def clean(v, tri, merge_pct=1.0, min_faces=64, min_diameter_pct=20.0, repair=True, jacobi=True):
    """The whole chain: a dict with vertices, indices, vertex_map, face_map, report, and the intermediate arrays.
    ``jacobi`` False skips the round count of the merge (report["merge_rounds"] is None): large inputs."""
    v, tri = np.asarray(v, dtype=f32), np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    V, F = v.shape[0], tri.shape[0]
    report = {k: 0 for k in REPORT_KEYS}
    if F == 0:
        report["unreferenced"] = V
        return {"vertices": v[:0], "indices": tri, "vertex_map": np.full(V, -1, dtype=np.int64),
                "face_map": np.zeros(0, dtype=np.int64), "report": report}
    used = check(v, tri)
    D = diagonal(v, used)
    report["unreferenced"] = int(V - used.sum())
    if merge_pct > 0:
        r = fraction(D, merge_pct)
        target = merge_targets(v, used, r)
        if jacobi:
            again, report["merge_rounds"] = merge_rounds(v, used, r)
            assert np.array_equal(again, target), "the two statements of the merge differ"
        else:
            report["merge_rounds"] = None
    else:
        target = np.where(used, np.arange(V), -1)
    report["merged"] = int((used & (target != np.arange(V))).sum())
    rel = target[tri]
    alive, akey = null_faces(v, rel)
    report["null_faces"] = int((~alive).sum())
    dup = duplicate_faces(rel, alive)
    report["duplicate_faces"] = int(dup.sum())
    alive = alive & ~dup
    label = components(rel, alive)
    removed, report["components"], report["components_removed"] = small_components(v, rel, alive, label, D, min_faces,
                                                                                   min_diameter_pct)
    report["component_faces_removed"] = int(removed.sum())
    alive = alive & ~removed
    root = None
    if repair:
        before = int(alive.sum())
        alive, report["edge_rounds"] = edge_rounds(rel, alive, akey)
        report["edge_faces_removed"] = before - int(alive.sum())
        root = fans(rel, alive)
    vertices, indices, vertex_map, face_map, report["vertices_split"] = emit(v, rel, alive, target, root)
    return {"vertices": vertices, "indices": indices, "vertex_map": vertex_map, "face_map": face_map, "report": report,
            "target": target, "label": label, "relabelled": rel, "diagonal": D}


# ---- what the cleaned mesh must satisfy, counted with numpy.unique ----------------------------------------------------------------

def edge_valences(tri):
    """the number of faces of each distinct edge"""
    tri = np.asarray(tri).reshape(-1, 3)
    e = np.sort(np.concatenate((tri[:, [1, 2]], tri[:, [2, 0]], tri[:, [0, 1]])), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1] if e.size else np.zeros(0, dtype=np.int64)


def fans_per_vertex(tri):
    """{vertex: number of fans}; a fan is a class of the faces of a vertex under sharing an edge incident to it"""
    tri = np.asarray(tri).reshape(-1, 3)
    faces_of = {}
    for f, row in enumerate(tri.tolist()):
        for x in row:
            faces_of.setdefault(x, []).append(f)
    out = {}
    for x, faces in faces_of.items():
        parent = {f: f for f in faces}

        def find(a):
            while parent[a] != a:
                a = parent[a]
            return a
        by_other = {}
        for f in faces:
            for y in tri[f].tolist():
                if y != x:
                    by_other.setdefault(y, []).append(f)
        for group in by_other.values():
            for g in group[1:]:
                parent[find(g)] = find(group[0])
        out[x] = len({find(f) for f in faces})
    return out


# ---- junk ---------------------------------------------------------------------------------------------------------------------

def append_mesh(v, tri, v2, tri2):
    return np.concatenate((v, v2)).astype(f32), np.concatenate((tri, np.asarray(tri2, dtype=np.int64) + v.shape[0]))


def strip(n, origin=(0.0, 0.0, 0.0), step=1.0, width=1.0):
    """a strip of n faces along x (a path of faces)"""
    k = n // 2 + 2
    x = np.arange(k) * step
    v = np.concatenate((np.stack((x, np.zeros(k), np.zeros(k)), axis=1), np.stack((x, np.full(k, width), np.zeros(k)), axis=1)))
    tri = []
    for i in range(k - 1):                                              # each face shares an edge with the next
        tri += [(i, i + 1, k + i), (i + 1, k + i + 1, k + i)]
    return (v + np.asarray(origin)).astype(f32), np.array(tri[:n], dtype=np.int64)


def book(pages, heights=None, origin=(0.0, 0.0, 0.0)):
    """`pages` triangles around one spine (0, 1); page k has its apex at height heights[k] in its own direction"""
    heights = list(heights) if heights is not None else [1.0 + k for k in range(pages)]
    v = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0)]
    tri = []
    for k in range(pages):
        a = 2.0 * math.pi * k / max(pages, 3) + 0.3
        v.append((0.5, heights[k] * math.cos(a), heights[k] * math.sin(a)))
        tri.append((0, 1, 2 + k))
    return (np.array(v) + np.asarray(origin)).astype(f32), np.array(tri, dtype=np.int64)


def cone(apex, n=5, radius=0.2, axis=(0.0, 0.0, 1.0), closed=True):
    """a fan of n faces around `apex` (vertex 0), its rim a circle at apex + axis; open: one face fewer"""
    axis = np.asarray(axis, dtype=np.float64)
    u = np.cross(axis, (1.0, 0.3, 0.2))
    u /= np.linalg.norm(u)
    w = np.cross(axis, u)
    w /= np.linalg.norm(w)
    ang = 2.0 * math.pi * np.arange(n) / n
    rim = np.asarray(apex) + axis + radius * (np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * w)
    v = np.concatenate((np.asarray(apex, dtype=np.float64)[None], rim))
    tri = [(0, 1 + i, 1 + (i + 1) % n) for i in range(n if closed else n - 1)]
    return v.astype(f32), np.array(tri, dtype=np.int64)


def two_edges(first, second, k=3.0):
    """Two non-manifold edges, (0, 1) and (1, 2), that share face 0 = (0, 1, 2) of area key k^2.  `first`: the heights of
    the further faces of (0, 1), a face of height h has the key h^2; `second`: those of (1, 2), with the key (k h)^2.
    Faces in the order: the shared one, those of `first`, those of `second`."""
    v = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, k, 0.0)]
    tri = [(0, 1, 2)]
    for h in first:
        v.append((0.5, 0.0, h))
        tri.append((0, 1, len(v) - 1))
    for h in second:
        v.append((1.0, 0.5 * k, h))
        tri.append((1, 2, len(v) - 1))
    return np.array(v, dtype=f32), np.array(tri, dtype=np.int64)


def pinch(v, tri, x, y):
    """name vertex x wherever y was named: the two fans meet in one vertex"""
    tri = tri.copy()
    tri[tri == y] = x
    return v, tri


def with_junk(v, tri, seed=0):
    """`v`, `tri` plus everything the cleaner has to remove or repair; every coordinate stays inside the original box
    stretched by a little, so the diagonal changes by a few percent at most.  Returns float32 vertices, int64 faces."""
    rng = np.random.RandomState(seed)
    v, tri = np.asarray(v, dtype=f32), np.asarray(tri, dtype=np.int64)
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    size = float(np.linalg.norm(hi - lo))
    F0 = tri.shape[0]
    # duplicated faces: rotated and reversed copies of a few faces
    picks = rng.choice(F0, 6, replace=False)
    tri = np.concatenate((tri, tri[picks[:3]][:, [1, 2, 0]], tri[picks[3:]][:, [2, 1, 0]]))
    # a null face: three vertices of one face's edge, one repeated
    tri = np.concatenate((tri, [[tri[0, 0], tri[0, 1], tri[0, 1]]]))
    # near-duplicate vertices: copies of a few vertices a hair away, used by a copy of one of their faces
    for f in rng.choice(F0, 4, replace=False):
        x = tri[f, 0]
        v = np.concatenate((v, (v[x].astype(np.float64) + 1e-4 * size * rng.uniform(-1, 1, 3))[None].astype(f32)))
        tri = np.concatenate((tri, [[v.shape[0] - 1, tri[f, 1], tri[f, 2]]]))
    # fragments: a 5-face strip and a small cone, away from the surface
    sv, st = strip(5, origin=hi + 0.02 * size, step=0.03 * size, width=0.03 * size)
    v, tri = append_mesh(v, tri, sv, st)
    cv, ct = cone(lo - 0.05 * size, n=6, radius=0.03 * size, axis=(0.0, 0.0, 0.03 * size))
    v, tri = append_mesh(v, tri, cv, ct)
    # a 3-page book: one more face on an interior edge of the surface
    a, b = int(tri[1, 0]), int(tri[1, 1])
    v = np.concatenate((v, (0.5 * (v[a].astype(np.float64) + v[b]) + (0.0, 0.0, 0.05 * size))[None].astype(f32)))
    tri = np.concatenate((tri, [[a, b, v.shape[0] - 1]]))
    # a pinched vertex: two far-apart vertices of the surface named as one
    surface = v[:int(tri[:F0].max()) + 1].astype(np.float64)
    far = int(np.argmax(((surface - surface[tri[5, 0]]) ** 2).sum(axis=1)))
    v, tri = pinch(v, tri, int(tri[5, 0]), far)
    # an unreferenced vertex
    v = np.concatenate((v, v[:1]))
    return v.astype(f32), tri.astype(np.int64)


# ---- the cases of the merge tests: points, each named by one face (i, i, i) ------------------------------------------------------

def points_mesh(p):
    p = np.asarray(p, dtype=np.float64)
    i = np.arange(p.shape[0])
    return p.astype(f32), np.stack((i, i, i), axis=1).astype(np.int64)


def line_case(n=200, shuffle=False, seed=2):
    """n points 0.6 r apart on the x axis, ascending (one vertex is decided per round) or shuffled: (v, tri, merge_pct)"""
    x = np.arange(n, dtype=np.float64) * 0.6
    if shuffle:
        x = x[np.random.RandomState(seed).permutation(n)]
    p = np.stack((x, np.zeros(n), np.zeros(n)), axis=1)
    return points_mesh(p) + (100.0 / (0.6 * (n - 1)),)                 # D = 0.6 (n - 1), so r = 1 up to its rounding


BOX_480 = np.array([[0.0, 0.0, 0.0], [160.0, 320.0, 320.0]])          # D = 480 exactly; merge_pct = 5 gives r = 24


def exact_case(scale=2.0 ** -7):
    """pairs at distance exactly r = 24 scale and one ulp beyond, integers times a power of two: (v, tri, merge_pct).
    Pair k is the vertices (2k, 2k + 1); pairs 0, 1 and 2 are close, pairs 3, 4 and 5 are not; no two pairs are close."""
    ulp = 2.0 ** -15                                                     # of a float32 in [256, 512)
    ends = [(24.0, 0.0, 0.0), (16.0, 16.0, 8.0), (0.0, 0.0, 24.0), (24.0 + ulp, 0.0, 0.0), (16.0, 16.0 + ulp, 8.0),
            (0.0, 0.0, 24.0 + ulp)]
    p = []
    for k, e in enumerate(ends):
        base = np.array([30.0 + 20.0 * k, 30.0 + 50.0 * k, 30.0 + 48.0 * k])
        p += [base, base + np.array(e)]
    return points_mesh(np.concatenate((np.array(p), BOX_480)) * scale) + (5.0,)


def cells_case():
    """26 close pairs, each straddling a cell face, edge or corner of the merge grid in its own direction; D = 100, r = 1"""
    p, k = [], 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == dy == dz == 0:
                    continue
                c = np.array([4.0 * (k % 5) + 4.0, 4.0 * ((k // 5) % 5) + 4.0, 4.0 * (k // 25) + 4.0])
                d = 0.25 * np.array([dx, dy, dz])
                p += [c - d, c + d]
                k += 1
    return points_mesh(np.concatenate((np.array(p), [[0.0, 0.0, 0.0], [36.0, 48.0, 80.0]]))) + (1.0,)


def ball_case(n=300, seed=4):
    """n points inside one ball of radius r / 2 (r = 1, D = 100): more than a workgroup in one cell, one centre: vertex 0"""
    rng = np.random.RandomState(seed)
    d = rng.normal(size=(n, 3))
    d *= (0.5 * rng.uniform(0, 1, n) ** (1 / 3) / np.linalg.norm(d, axis=1))[:, None]
    return points_mesh(np.concatenate((d + (18.5, 24.5, 40.5), [[0.0, 0.0, 0.0], [36.0, 48.0, 80.0]]))) + (1.0,)


def cloud_case(n, seed=6):
    """n random points of the unit cube with r of about 0.14"""
    return points_mesh(np.random.RandomState(seed + n).uniform(0, 1, (n, 3))) + (8.0,)
