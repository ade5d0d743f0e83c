"""The definitions of include/gd_mesh_geometry.h stated in torch on the CPU, parameterised by dtype, for
tests/test_mesh_geometry_cpu.py (which pins this file) and tests/test_mesh_geometry_gpu.py (which compares the kernels with
its float64 evaluation and takes its allowance from its float32 evaluation).

Two forms.  The scatter forms (``index_add``, sequential on the CPU) serve every mesh size and carry autograd; they sum in
face / edge order, not in the kernels' gather order.  The ``*_looped`` / ``*_dense`` forms restate the same definitions
with Python loops and a dense matrix; the CPU test holds the two against each other on small meshes.  ``edges_numpy`` and
``connected_faces_numpy`` state the connectivity with dictionaries."""
import numpy as np
import torch

NORM_EPS = 1e-12     # torch.nn.functional.normalize
COS_EPS = 1e-8       # torch.cosine_similarity


# ---- meshes --------------------------------------------------------------------------------------------------------------

def tube(nu, nv, r=0.3, h=1.0):
    """(vertices float64 [(nv + 1) nu, 3], triangles int64 [2 nu nv, 3]) of an open tube around z."""
    ang = 2.0 * np.pi * np.arange(nu) / nu
    v = np.array([[r * np.cos(a), r * np.sin(a), h * j / nv] for j in range(nv + 1) for a in ang], dtype=np.float64)
    q = np.array([[j * nu + i, j * nu + (i + 1) % nu, (j + 1) * nu + (i + 1) % nu, (j + 1) * nu + i]
                  for j in range(nv) for i in range(nu)], dtype=np.int64)
    return v, np.concatenate((q[:, [0, 1, 2]], q[:, [0, 2, 3]]))


def fan(n, r=0.5):
    """n triangles around vertex 0 (valence n + 1 > a wave's 64 lanes for n = 100): an open fan of angle 5 rad."""
    ang = 5.0 * np.arange(n + 1) / n
    rim = np.stack((r * np.cos(ang), r * np.sin(ang), 0.05 * np.sin(3 * ang)), axis=1)
    v = np.concatenate((np.zeros((1, 3)), rim))
    tri = np.array([[0, 1 + i, 2 + i] for i in range(n)], dtype=np.int64)
    return v, tri


SINGLE = (np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 0.9, 0.3]]), np.array([[0, 1, 2]], dtype=np.int64))
QUAD = (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.1], [1.1, 1.0, 0.0], [0.0, 0.9, 0.2]]),
        np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int64))


def noisy(v, sigma=0.01, seed=0):
    """``v`` plus seeded N(0, sigma) noise, rounded to float32 (the input both the kernels and the reference see)."""
    return (v + np.random.RandomState(seed).normal(0.0, sigma, size=v.shape)).astype(np.float32)


# ---- connectivity, in numpy ----------------------------------------------------------------------------------------------

def _edge_faces(tri):
    faces = {}
    for f, (a, b, c) in enumerate(np.asarray(tri).tolist()):
        for p, q in ((b, c), (c, a), (a, b)):              # edge i lies between corners i + 1 and i + 2
            faces.setdefault((min(p, q), max(p, q)), []).append(f)
    return faces


def edges_numpy(tri):
    """int64 [E,2]: the distinct undirected edges, each row sorted, rows sorted."""
    return np.array(sorted(_edge_faces(tri)), dtype=np.int64).reshape(-1, 2)


def connected_faces_numpy(tri):
    """int64 [P,2]: (f, g), f < g, once for every edge that exactly the two faces f and g share; rows sorted."""
    pairs = [(min(fs), max(fs)) for fs in _edge_faces(tri).values() if len(fs) == 2 and fs[0] != fs[1]]
    return np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)


def face_neighbours_numpy(tri):
    """int64 [F,3]: the face across edge i, -1 unless exactly two faces share that edge."""
    faces = _edge_faces(tri)
    out = -np.ones((len(tri), 3), dtype=np.int64)
    for f, (a, b, c) in enumerate(np.asarray(tri).tolist()):
        for i, (p, q) in enumerate(((b, c), (c, a), (a, b))):
            fs = faces[(min(p, q), max(p, q))]
            if len(fs) == 2 and fs[0] != fs[1]:
                out[f, i] = fs[1] if fs[0] == f else fs[0]
    return out


def neighbours_numpy(tri, V):
    """list of V ascending lists: the vertices sharing an edge with each vertex."""
    nbr = [set() for _ in range(V)]
    for p, q in _edge_faces(tri):
        if p != q:
            nbr[p].add(q)
            nbr[q].add(p)
    return [sorted(s) for s in nbr]


# ---- the definitions, scatter form (any size, autograd) --------------------------------------------------------------------

def _t(a, dtype):
    return a.to(dtype) if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=dtype)


def normalize(x, eps=NORM_EPS):
    return x / torch.clamp(torch.sqrt((x * x).sum(-1, keepdim=True)), min=eps)


def normals(v, tri):
    """(fn [F,3], vn [V,3]) of vertices ``v`` (tensor, any float dtype) and triangles ``tri`` (int array)."""
    tri = torch.as_tensor(np.asarray(tri), dtype=torch.int64)
    a, b, c = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    fn = normalize(torch.linalg.cross(b - a, c - a))
    s = torch.zeros_like(v)
    for i in range(3):
        s = s.index_add(0, tri[:, i], fn)
    return fn, normalize(s)


def laplacian_terms(v, tri):
    """[V]: |delta_i|^2 with delta_i = mean of the edge neighbours - v_i (-v_i for a vertex without an edge)."""
    V = v.shape[0]
    e = edges_numpy(tri)
    e = torch.as_tensor(e[e[:, 0] != e[:, 1]], dtype=torch.int64)
    src, dst = torch.cat((e[:, 0], e[:, 1])), torch.cat((e[:, 1], e[:, 0]))
    deg = torch.zeros(V, dtype=v.dtype).index_add(0, src, torch.ones(src.shape[0], dtype=v.dtype))
    s = torch.zeros_like(v).index_add(0, src, v[dst])
    delta = torch.where(deg[:, None] > 0, s / torch.clamp(deg, min=1)[:, None], torch.zeros_like(s)) - v
    return (delta * delta).sum(-1)


def laplacian_loss(v, tri):
    return laplacian_terms(v, tri).sum() / v.shape[0]


def consistency_terms(fn, tri):
    """[P]: (1 - cos)^2 of each pair of connected_faces_numpy(tri)."""
    pairs = torch.as_tensor(connected_faces_numpy(tri), dtype=torch.int64)
    f, g = fn[pairs[:, 0]], fn[pairs[:, 1]]
    mf = torch.clamp(torch.sqrt((f * f).sum(-1)), min=COS_EPS)
    mg = torch.clamp(torch.sqrt((g * g).sum(-1)), min=COS_EPS)
    cos = (f * g).sum(-1) / (mf * mg)
    return (1 - cos) ** 2


def consistency_loss(fn, tri):
    """Mean of the terms; 0 for a mesh without a pair (the header's choice; the reference's mean over nothing is NaN)."""
    terms = consistency_terms(fn, tri)
    return terms.sum() / terms.shape[0] if terms.shape[0] else terms.sum()


def scalar_sums(terms):
    """Three float sums of one array of terms: torch's, ascending sequential, descending sequential.  A float32 scalar is a
    single sample of a rounding walk and can be exact by chance; the float32 reference's error of a LOSS is therefore taken
    as the largest over these three orders."""
    return [terms.sum(), torch.cumsum(terms, 0)[-1], torch.cumsum(terms.flip(0), 0)[-1]] if terms.shape[0] else [terms.sum()]


# ---- the same definitions with loops and a dense matrix (small meshes; pins the scatter forms) ----------------------------

def normals_looped(v, tri):
    tri = np.asarray(tri)
    fn = []
    for a, b, c in tri.tolist():
        u, w = v[b] - v[a], v[c] - v[a]
        cr = torch.stack((u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]))
        fn.append(cr / max(float(torch.sqrt((cr * cr).sum())), NORM_EPS))
    fn = torch.stack(fn) if fn else torch.zeros((0, 3), dtype=v.dtype)
    vn = []
    for i in range(v.shape[0]):
        s = torch.zeros(3, dtype=v.dtype)
        for f in range(len(tri)):
            for k in range(3):
                if tri[f, k] == i:
                    s = s + fn[f]
        vn.append(s / max(float(torch.sqrt((s * s).sum())), NORM_EPS))
    return fn, torch.stack(vn)


def laplacian_dense(tri, V, dtype):
    """The reference's matrix: L[i, j] = 1 / deg(i) for an edge (i, j), L[i, i] = -1."""
    L = torch.zeros((V, V), dtype=dtype)
    for i, ns in enumerate(neighbours_numpy(tri, V)):
        for j in ns:
            L[i, j] = 1.0 / len(ns)
        L[i, i] = -1.0
    return L


def laplacian_loss_dense(v, tri):
    d = laplacian_dense(tri, v.shape[0], v.dtype) @ v
    return (torch.sqrt((d * d).sum(1)) ** 2).mean()


def consistency_loss_looped(fn, tri):
    nbr = face_neighbours_numpy(tri)
    total, P = torch.zeros((), dtype=fn.dtype), 0
    for f in range(len(nbr)):
        for i in range(3):
            g = int(nbr[f, i])
            if g > f:
                cos = torch.nn.functional.cosine_similarity(fn[f][None], fn[g][None], dim=1, eps=COS_EPS)[0]
                total = total + (1 - cos) ** 2
                P += 1
    return total / P if P else total


def normalised_error(g, g64):
    """max |g - g64| / max |g64|"""
    g64 = np.asarray(g64, dtype=np.float64)
    return float(np.abs(np.asarray(g, dtype=np.float64) - g64).max() / np.abs(g64).max())
