"""The statement of the final-mesh post-process (tests/simplify_reference.py) on the CPU: what a decimation keeps, where it
ends when it runs to exhaustion, that quadrics measure what they should, Taubin smoothing, the OBJ writer and the rotation;
and what of garmentdreamer_amd/mesh_simplify.py needs no GPU."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import remesh_reference as rr
from tests import simplify_reference as sr

TARGETS = ["half", "quarter", "exhaustion"]
# faces left when nothing more may collapse (passes = 4).  An open mesh ends without interior vertices, so F = B - 2 chi with
# B boundary vertices; a closed one ends as a tetrahedron; a tetrahedron, a lone triangle and a two-triangle quad stay.
EXHAUSTED = {"single": 1, "quad": 2, "cloth": 38, "tube": 48, "sphere": 4, "cloth_extra": 38, "tetrahedron": 4,
             "octahedron": 4, "integer": 22, "folded": 46}


def target_of(name, kind):
    F = sr.mesh(name)[1].shape[0]
    return {"half": F // 2, "quarter": F // 4, "exhaustion": 2}[kind]


@functools.lru_cache(maxsize=None)
def decimated(name, kind):
    """(vertices, triangles, info) of the statement; shared and read-only"""
    v, tri = sr.mesh(name)
    return sr.decimate(v, tri, target_of(name, kind))


@pytest.mark.parametrize("kind", TARGETS)
@pytest.mark.parametrize("name", sr.MESHES)
def test_decimation_of_the_statement(name, kind):
    v, tri = sr.mesh(name)
    sv, stri = rr.compact_vertices(v, tri)
    target = target_of(name, kind)
    v2, t2, info = decimated(name, kind)
    print(f"{name} {kind}: faces {tri.shape[0]} -> {t2.shape[0]} (target {target}), rounds {len(info['selected'])}, "
          f"reached {info['reached']}")
    assert v2.dtype == np.float32
    if tri.shape[0] <= target:
        assert np.array_equal(v2, v) and np.array_equal(t2, tri) and info == {"reached": True, "selected": [], "faces": []}
        return
    assert rr.invariants(v2, t2) == rr.invariants(sv, stri)            # manifold, oriented, no duplicate face, every
    rows = {p.tobytes() for p in sv}                                   # vertex referenced; Euler and boundary loops kept
    assert all(p.tobytes() in rows for p in v2)                        # every output position is bitwise an input position
    assert sr.boundary_of(v2, t2) == sr.boundary_of(sv, stri)          # boundary vertices, positions and edges
    assert info["faces"][-1] == t2.shape[0] and len(info["faces"]) == len(info["selected"])
    assert all(a - 2 * n == b for a, n, b in zip([tri.shape[0]] + info["faces"], info["selected"], info["faces"]))
    assert info["reached"] == (t2.shape[0] <= target)
    if info["reached"]:
        assert target - 1 <= t2.shape[0] <= target
    else:
        assert info["selected"][-1] == 0


@pytest.mark.parametrize("name", sr.MESHES)
def test_exhaustion(name):
    v, tri = sr.mesh(name)
    v2, t2, info = decimated(name, "exhaustion")
    assert t2.shape[0] == EXHAUSTED[name]
    c = rr.Connectivity(t2, v2.shape[0])
    chi, loops = rr.invariants(v2, t2)
    if loops:
        assert not (~c.bnd).any() and t2.shape[0] == int(c.bnd.sum()) - 2 * chi
    else:
        assert v2.shape[0] == 4
    if name in ("single", "quad", "tetrahedron"):
        assert np.array_equal(v2, v) and np.array_equal(t2, tri)


@pytest.mark.parametrize("name", ["cloth", "tube", "sphere", "folded"])
def test_a_vertex_lies_on_its_own_quadric(name):
    v, tri = sr.mesh(name)
    c = rr.Connectivity(tri, v.shape[0])
    q, p = sr.vertex_quadrics(v, c), v.astype(np.float64)
    worst = 0.0
    for x in range(c.V):
        size = 0.0
        for t in sr.quadric_terms(q[x], p[x]):
            size = size + abs(t)
        value = abs(sr.quadric_value(q[x], p[x]))
        assert size > 0.0 or value == 0.0                              # a vertex at the origin of a flat patch: all zeros
        worst = max(worst, value / size if size > 0.0 else 0.0)
    print(name, "largest |Q_v(p_v)| / sum of |terms|", worst)
    assert worst <= 1e-12


def _exact_quadrics(v, tri):
    """the vertex quadrics of an integer mesh in Python integers"""
    p = [[int(x) for x in row] for row in v]
    q = [[0] * 10 for _ in p]
    for t in tri.tolist():
        p0, p1, p2 = (p[x] for x in t)
        u, w = [p1[i] - p0[i] for i in range(3)], [p2[i] - p0[i] for i in range(3)]
        n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
        assert any(n), "a degenerate face"
        d = -(n[0] * p0[0] + n[1] * p0[1] + n[2] * p0[2])
        fq = [n[0] * n[0], n[0] * n[1], n[0] * n[2], n[0] * d, n[1] * n[1], n[1] * n[2], n[1] * d, n[2] * n[2], n[2] * d, d * d]
        for x in t:
            q[x] = [a + b for a, b in zip(q[x], fq)]
    return p, q


def test_the_integer_mesh_is_exact():
    v, tri = sr.mesh("integer")
    assert np.array_equal(v, np.round(v)) and v[:, 2].min() == 0 and v[:, 2].max() == 4
    c = rr.Connectivity(tri, v.shape[0])
    p, q = _exact_quadrics(v, tri)
    got = sr.vertex_quadrics(v, c)
    assert got.tolist() == q
    keys, direction, costs = sr.candidates(c, v.astype(np.float64), got)
    for e, (lo, hi) in enumerate(c.ev.tolist()):
        for s, (a, b) in enumerate(((lo, hi), (hi, lo))):
            s_ = [x + y for x, y in zip(q[a], q[b])]
            x, y, z = p[b]
            exact = (s_[0] * x * x + s_[4] * y * y + s_[7] * z * z + 2 * (s_[1] * x * y + s_[2] * x * z + s_[5] * y * z)
                     + 2 * (s_[3] * x + s_[6] * y + s_[8] * z) + s_[9])
            assert exact >= 0 and costs[e, s] == exact and exact < 1 << 24   # the key's fp32 bits hold the cost exactly
    live = [k >> 32 for k in keys if k != sr.NO_KEY]
    assert len(set(live)) < len(live)                                  # equal costs: the edge index decides


def _distances(v, tri, v2, t2):
    d2 = rr.closest_on_surface(v.astype(np.float64), v2.astype(np.float64), t2)[1]
    total = 0.0
    for x in d2:
        total = total + float(x)
    return float(np.sqrt(d2.max())), float(np.sqrt(total / d2.shape[0]))


def test_quadrics_keep_the_folded_sheet_better_than_edge_length():
    v, tri = sr.mesh("folded")
    target = tri.shape[0] // 3
    vq, tq, iq = sr.decimate(v, tri, target)
    vl, tl, il = sr.decimate(v, tri, target, cost="length")
    assert iq["reached"] and il["reached"]
    (qmax, qrms), (lmax, lrms) = _distances(v, tri, vq, tq), _distances(v, tri, vl, tl)
    print(f"folded sheet {tri.shape[0]} -> {tq.shape[0]} / {tl.shape[0]} faces: quadric max {qmax:.5f} rms {qrms:.5f}; "
          f"length max {lmax:.5f} rms {lrms:.5f}")
    assert qmax < lmax and qrms < lrms


# ---- Taubin smoothing -----------------------------------------------------------------------------------------------------

def noisy_sphere():
    v, tri = rr.sphere(3, stretch=1.0)
    noise = np.random.RandomState(11).normal(0.0, 0.03, v.shape[0])
    return (v.astype(np.float64) * (1.0 + noise)[:, None]).astype(np.float32), tri


def _radial(v):
    r = np.sqrt(rr.dot(v.astype(np.float64), v.astype(np.float64)))
    return float(r.mean()), float(r.std())


def test_taubin_float32_and_float64_statements_agree():
    for v, tri in (noisy_sphere(), sr.mesh("tube"), sr.mesh("cloth")):
        a, b = sr.taubin(v, tri, dtype=np.float64), sr.taubin(v, tri, dtype=np.float32)
        c = rr.Connectivity(tri, v.shape[0])
        # 20 passes; a pass rounds at most deg + 4 times per component, each by 2^-24 of a magnitude below max |v| (the
        # running sum by deg times that, divided by deg again); an error made in a lam pass grows by at most
        # |1 - 2 mu| = 2.06 in the mu pass that follows, and a whole step does not amplify ((1 - lam k)(1 - mu k) <= 1.001)
        bound = 20 * (int(np.diff(c.nbr_ptr).max()) + 4) * 2.0 ** -24 * 2.06 * float(np.abs(v).max())
        err = float(np.abs(a - b.astype(np.float64)).max())
        print("taubin float32 against float64:", err, "bound", bound)
        assert b.dtype == np.float32 and err <= bound


def test_taubin_removes_noise_and_shrinks_less_than_laplacian_smoothing():
    v, tri = noisy_sphere()
    c = rr.Connectivity(tri, v.shape[0])
    mean0, dev0 = _radial(v)
    devs, x = [dev0], v.astype(np.float64)
    for _ in range(10):
        x = sr.smooth_pass(sr.smooth_pass(x, c, np.float32(0.5)), c, np.float32(-0.53))
        devs.append(_radial(x)[1])
    print("rms radial deviation per step", devs)
    assert all(b < a for a, b in zip(devs, devs[1:]))
    assert np.array_equal(x, sr.taubin(v, tri))
    y = v.astype(np.float64)
    for _ in range(10):
        y = sr.smooth_pass(y, c, np.float32(0.5))
    print("mean radius", mean0, "taubin", _radial(x)[0], "ten lam passes", _radial(y)[0])
    assert abs(_radial(x)[0] - mean0) < abs(_radial(y)[0] - mean0)


def test_taubin_keeps_the_rims_of_the_tube_in_their_planes():
    v, tri = sr.mesh("tube")
    c = rr.Connectivity(tri, v.shape[0])
    for dtype in (np.float32, np.float64):
        out = sr.taubin(v, tri, dtype=dtype)
        assert set(v[c.bnd, 2].tolist()) == {0.0, 1.0} and np.array_equal(out[c.bnd, 2], v[c.bnd, 2].astype(dtype))
        assert not np.array_equal(out[c.bnd, :2], v[c.bnd, :2].astype(dtype))     # it does move, along the rim
        assert not np.array_equal(out[~c.bnd], v[~c.bnd].astype(dtype))


# ---- rotation and the OBJ writer --------------------------------------------------------------------------------------------

def test_the_rotation_is_exact():
    v, _ = sr.mesh("tube")
    r = sr.rotate(v)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(bits(r[:, 0]), bits(v[:, 0])) and np.array_equal(bits(r[:, 1]), bits(v[:, 2]))
    assert np.array_equal(bits(r[:, 2]), bits(-v[:, 1]))
    assert np.array_equal(bits(sr.rotate(sr.rotate(sr.rotate(r)))), bits(v))
    angle = np.radians(-90.0)                                           # the reference's matrix, up to its cos(-pi/2) = 6e-17
    m = np.array([[1, 0, 0], [0, np.cos(angle), -np.sin(angle)], [0, np.sin(angle), np.cos(angle)]])
    assert np.abs(v.astype(np.float64) @ m.T - r).max() <= 1e-15


def test_write_obj_reads_back_the_same_bits(tmp_path):
    from garmentdreamer_amd import mesh_simplify as ms
    from garmentdreamer_amd import template
    v, tri = sr.mesh("sphere")
    v = v.copy()
    v[0] = (-0.0, 1e-30, 16777217.0)
    v[1] = (np.float32(1.0) / np.float32(3.0), np.float32(3.4e38), np.float32(1e-45))
    for vertices, indices in ((v, tri), (torch.from_numpy(v), torch.from_numpy(tri.astype(np.int32)))):
        path = str(tmp_path / "mesh.obj")
        ms.write_obj(path, vertices, indices)
        v2, t2 = template.load_obj(path)
        assert np.array_equal(v2.astype(np.float32).view(np.uint32), v.view(np.uint32)) and np.array_equal(t2, tri)
        assert set(line.split()[0] for line in open(path)) == {"v", "f"}
    with pytest.raises(ValueError, match="not finite"):
        ms.write_obj(str(tmp_path / "bad.obj"), np.full((3, 3), np.nan, np.float32), tri[:1] * 0 + [[0, 1, 2]])
    with pytest.raises(ValueError, match="out of range"):
        ms.write_obj(str(tmp_path / "bad.obj"), v[:3], np.array([[0, 1, 3]]))


# ---- the package, without a GPU -----------------------------------------------------------------------------------------------

def test_the_statement_refuses_what_the_kernels_refuse():
    v, tri = sr.mesh("quad")
    fan = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    with pytest.raises(ValueError, match="non-manifold"):
        sr.decimate(np.zeros((5, 3), np.float32), fan, 1)
    with pytest.raises(ValueError, match="out of range"):
        sr.decimate(v, np.array([[0, 1, 4]]), 0)
    with pytest.raises(ValueError, match="twice"):
        sr.decimate(v, np.array([[0, 1, 1]]), 0)
    with pytest.raises(ValueError, match="target_faces"):
        sr.decimate(v, tri, -1)
    with pytest.raises(ValueError, match="passes"):
        sr.decimate(v, tri, 1, passes=0)


def test_cpu_tensors_are_refused():
    from garmentdreamer_amd import mesh_simplify as ms
    v, tri = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for call in (lambda: ms.decimate_quadric(v, tri, 1), lambda: ms.taubin_smooth(v, tri), lambda: ms.rotate_upright(v),
                 lambda: ms.post_process_mesh(v, tri)):
        with pytest.raises(ValueError, match="no CPU path"):
            call()


def test_the_bindings_cover_the_header():
    from garmentdreamer_amd import _native
    from garmentdreamer_amd.deformer import Deformer
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gd_mesh_simplify.h")).read()
    declared = set(re.findall(r"^int (gd_mesh_simplify_\w+)\(", header, flags=re.M))
    assert declared == set(_native.MESH_SIMPLIFY_SIGNATURES) and len(declared) == 6
    L = _native.lib()
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_mesh_simplify.h but not exported"
        assert _native.error_channel(name) == "gd_mesh_last_error"
        count = len(re.search(name + r"\((.*?)\);", header, flags=re.S).group(1).split(","))
        assert count == len(_native.MESH_SIMPLIFY_SIGNATURES[name][1]), name
    assert L.gd_mesh_simplify_rotate(None, 0, None, None) == -1 and b"simplify rotate" in L.gd_mesh_last_error()
    assert L.gd_mesh_simplify_quadrics(None, None, None) == -1 and b"simplify quadrics" in L.gd_mesh_last_error()
    assert hasattr(Deformer, "final_mesh")
