"""The remesher's statement (tests/remesh_reference.py) on the CPU: the invariants of a whole remesh on every test mesh, the
decision margins that let the float64 statement and the fp32 kernels decide alike, and the argument validation of
garmentdreamer_amd/mesh_remesh.py that needs no GPU."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_geometry_reference as gref
from tests import remesh_reference as rr

WHOLE = [(name, 0.5) for name in rr.MESHES] + [("tube", 1.4), ("cloth", 1.5)]
MIN_MARGIN = 1e-5     # some thirty times the fp32 rounding of a squared edge length formed from float32 inputs


@functools.lru_cache(maxsize=None)
def _remeshed(name, factor, dtype):
    v, tri = rr.mesh(name)
    sv, stri = rr.compact_vertices(v, tri)
    h = factor * rr.mean_edge_length(sv, stri)
    return (sv, stri, h) + rr.remesh(v, tri, h, dtype=dtype)


def test_the_tiny_meshes_are_those_of_the_geometry_tests():
    for mine, theirs in ((rr.SINGLE, gref.SINGLE), (rr.QUAD, gref.QUAD)):
        assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])


@pytest.mark.parametrize("name,factor", WHOLE)
def test_whole_remesh_of_the_statement(name, factor):
    sv, stri, h, v, tri, info, margins = _remeshed(name, factor, np.float64)
    chi0, loops0 = rr.invariants(sv, stri)
    chi, loops = rr.invariants(v, tri)        # <= 2 faces per edge, no repeated vertex, no duplicate face, every vertex
    assert (chi, loops) == (chi0, loops0)     # referenced, consistent orientation, finite; Euler and loops kept
    print(f"{name} x{factor}: faces {stri.shape[0]} -> {tri.shape[0]}, margins {margins.smallest}")
    print(f"   longest edge after the last split {info['longest_after_split'][-1]:.4f} h; a projection moved a vertex by at "
          f"most {info['moved_most']:.4f} h; quality {rr.quality(v, tri, h)}")
    assert info["longest_after_split"][-1] <= 4.0 / 3.0
    assert sum(info["unprojected"]) == 0
    d = float(np.sqrt(rr.closest_on_surface(v, sv.astype(np.float64), stri)[1].max()))
    assert d <= 1e-12 * h
    assert margins.minimum() >= MIN_MARGIN
    if name not in ("single", "quad"):
        assert sum(info["split"]) > 0 and sum(info["collapsed"]) > 0 and sum(info["flipped"]) > 0


@pytest.mark.parametrize("name,factor", WHOLE)
def test_float32_and_float64_statements_decide_alike(name, factor):
    t64, t32 = _remeshed(name, factor, np.float64)[4], _remeshed(name, factor, np.float32)[4]
    assert np.array_equal(t64, t32)
    share = [rr.quality(*_remeshed(name, factor, dt)[3:5], _remeshed(name, factor, dt)[2]) for dt in (np.float64, np.float32)]
    print(name, factor, "quality float64", share[0], "float32", share[1])
    assert abs(share[0][0] - share[1][0]) <= rr.QUALITY_MARGIN["share"] / 2
    assert abs(share[0][1] - share[1][1]) <= rr.QUALITY_MARGIN["valence"] / 2


def test_single_pass_margins():
    """the single passes the GPU test compares exactly: split at 0.5 mean, a collapse round at 1.5 mean, a flip round on
    ``flip_test_mesh``"""
    for name in rr.MESHES:
        v, tri = rr.mesh(name)
        v, tri = rr.compact_vertices(v, tri)
        mean = rr.mean_edge_length(v, tri)
        m = rr.Margins()
        rr.split(v.astype(np.float64), tri, 0.5 * mean, m)
        rr.collapse_round(v.astype(np.float64), tri, 1.5 * mean, m)
        print(name, m.smallest)
        assert m.minimum() >= MIN_MARGIN
    v2, t2 = rr.flip_test_mesh()
    m = rr.Margins()
    _, flipped = rr.flip_round(v2.astype(np.float64), t2, m)
    print("fine cloth: flipped", flipped, m.smallest)
    assert flipped > 0 and m.minimum() >= MIN_MARGIN


def test_the_statement_refuses_what_the_kernels_refuse():
    v = rr.SINGLE[0].astype(np.float32)
    fan = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]])
    with pytest.raises(ValueError, match="non-manifold"):
        rr.remesh(np.zeros((5, 3), np.float32), fan, 0.5)
    with pytest.raises(ValueError, match="out of range"):
        rr.remesh(v, np.array([[0, 1, 3]]), 0.5)
    with pytest.raises(ValueError, match="twice"):
        rr.remesh(v, np.array([[0, 1, 1]]), 0.5)


def test_closest_point_regions():
    a, b, c = (np.array([x], dtype=np.float64) for x in ([0, 0, 0], [1, 0, 0], [0, 1, 0]))
    queries = np.array([[-1, -1, 1], [2, -0.5, 0], [-0.5, 2, 0], [0.5, -1, 2], [-1, 0.5, 0], [1, 1, 3], [0.25, 0.25, 5]], dtype=np.float64)
    want = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0, 0], [0, 0.5, 0], [0.5, 0.5, 0], [0.25, 0.25, 0]], dtype=np.float64)
    assert np.allclose(rr.closest_on_triangles(queries, a, b, c)[:, 0], want, atol=1e-15)


# ---- argument validation of the package, no GPU -----------------------------------------------------------------------------

def test_cpu_tensors_are_refused():
    from garmentdreamer_amd import mesh_remesh as mr
    v, tri = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for call in (lambda: mr.remesh_botsch(v, tri, 0.5), lambda: mr.split_long_edges(v, tri, 0.5),
                 lambda: mr.collapse_short_edges_round(v, tri, 0.5), lambda: mr.flip_edges_round(v, tri),
                 lambda: mr.tangential_relax(v, tri), lambda: mr.build_surface_grid(v, tri),
                 lambda: mr.project_to_surface(v, None), lambda: mr.compact_vertices(v, tri),
                 lambda: mr.mean_edge_length(v, None)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


@pytest.mark.parametrize("h", [0.0, -1.0, float("inf"), float("nan")])
def test_a_bad_target_is_a_value_error(h):
    from garmentdreamer_amd import mesh_remesh as mr
    with pytest.raises(ValueError, match="h must be positive and finite"):
        mr._target("remesh_botsch", h)


def test_the_bindings_cover_the_header():
    import os
    import re
    from garmentdreamer_amd import _native
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gd_mesh_remesh.h")).read()
    declared = set(re.findall(r"^int (gd_mesh_remesh_\w+)\(", header, flags=re.M))
    assert declared == set(_native.MESH_REMESH_SIGNATURES) and len(declared) == 20
    for name in declared:
        assert _native.error_channel(name) == "gd_mesh_last_error"
    assert hasattr(__import__("garmentdreamer_amd.deformer", fromlist=["Deformer"]).Deformer, "remesh")
