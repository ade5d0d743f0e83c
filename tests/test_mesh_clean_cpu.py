"""The statement of mesh cleaning (tests/clean_reference.py) on the CPU, against facts it does not restate: closeness pairs
from a k-d tree, components from scipy's graph search, edge valences and fans counted with numpy.unique; and what of
garmentdreamer_amd/mesh_clean.py needs no GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

from tests import clean_reference as cr
from tests import remesh_reference as rr
from tests import simplify_reference as sr

MERGE_CASES = {"line": lambda: cr.line_case(200), "shuffled": lambda: cr.line_case(200, shuffle=True), "exact": cr.exact_case,
               "cells": cr.cells_case, "ball": cr.ball_case, "cloud1": lambda: cr.cloud_case(1),
               "cloud63": lambda: cr.cloud_case(63), "cloud257": lambda: cr.cloud_case(257)}


def close_pairs(v, used, r):
    """The set of close pairs (a < b) among the used vertices: candidates from a k-d tree with a wider radius, each decided
    by the header's fp32 predicate one pair at a time."""
    ids = np.flatnonzero(used)
    tree = cKDTree(v[ids].astype(np.float64))
    r2 = np.float32(r) * np.float32(r)
    out = set()
    for i, j in tree.query_pairs(float(r) * 1.001 + 1e-30):
        a, b = int(ids[i]), int(ids[j])
        d = v[a] - v[b]
        if cr.sq3(d[0], d[1], d[2]) <= r2:
            out.add((min(a, b), max(a, b)))
    return out


@pytest.mark.parametrize("name", sorted(MERGE_CASES))
def test_merge_statement(name):
    v, tri, pct = MERGE_CASES[name]()
    used = cr.check(v, tri)
    r = cr.fraction(cr.diagonal(v, used), pct)
    target = cr.merge_targets(v, used, r)
    again, rounds = cr.merge_rounds(v, used, r)
    assert np.array_equal(target, again)                               # the sequential and the round statements agree
    pairs = close_pairs(v, used, r)
    centres = set(np.flatnonzero(target == np.arange(v.shape[0])).tolist())
    assert not any(a in centres and b in centres for a, b in pairs)    # no two centres are close
    for x in np.flatnonzero(used & (target != np.arange(v.shape[0]))):
        t = int(target[x])
        assert t in centres and (min(x, t), max(x, t)) in pairs        # every vertex is close to its target
        assert t == min(c for c in centres if (min(c, x), max(c, x)) in pairs)      # and its target is the lowest close centre
    print(name, "rounds", rounds, "centres", len(centres), "pairs", len(pairs))
    if name == "line":
        assert rounds == 200
    if name == "shuffled":
        assert rounds < 20
    if name == "ball":
        assert (target[:300] == 0).all() and rounds == 2
    if name == "exact":
        assert float(r) == 24.0 * 2.0 ** -7 and target[:12].tolist() == [0, 0, 2, 2, 4, 4, 6, 7, 8, 9, 10, 11]
    if name == "cells":
        assert target[:52].tolist() == [2 * (i // 2) for i in range(52)]


def test_jacobi_round_counts_of_a_grid():
    g = np.arange(24, dtype=np.float64)
    x, y = np.meshgrid(g, g, indexing="xy")
    rng = np.random.RandomState(1)
    p = np.stack((x + rng.uniform(-0.1, 0.1, x.shape), y + rng.uniform(-0.1, 0.1, x.shape), 0 * x), axis=-1).reshape(-1, 3)
    v, tri = cr.points_mesh(p)
    used = cr.check(v, tri)
    for r, most in ((1.5, 24 * 24), (0.5, 1)):
        target, rounds = cr.merge_rounds(v, used, np.float32(r))
        assert np.array_equal(target, cr.merge_targets(v, used, np.float32(r))) and 1 <= rounds <= most
        print("24 x 24 row-major grid, r =", r, "spacings:", rounds, "rounds")
        assert rounds == 1 or r > 1


# ---- test meshes ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dirty(name):
    if name == "sheet":
        return cr.with_junk(*sr.folded_sheet())
    if name == "tube":
        return cr.with_junk(*rr.jittered_tube())
    if name == "cloth_heavy":
        return rr.cloth(10)
    if name == "book4":
        return cr.book(4, heights=[3.0, 1.0, 4.0, 2.0])
    if name == "book6":
        return cr.book(6)
    v, tri = cr.cone((0.0, 0.0, 0.0))
    cv, ct = cr.cone((0.0, 0.0, 0.0), axis=(0.0, 1.0, -0.5))
    return cr.pinch(*cr.append_mesh(v, tri, cv, ct), 0, v.shape[0])     # "cones"


ARGS = {"sheet": dict(min_faces=32, min_diameter_pct=10.0), "tube": dict(min_faces=32, min_diameter_pct=10.0),
        "cloth_heavy": dict(merge_pct=14.0, min_faces=0, min_diameter_pct=0.0), "book4": dict(min_faces=0, min_diameter_pct=0.0),
        "book6": dict(min_faces=0, min_diameter_pct=0.0), "cones": dict(min_faces=0, min_diameter_pct=0.0)}


@functools.lru_cache(maxsize=None)
def cleaned(name):
    v, tri = dirty(name)
    return cr.clean(v, tri, **ARGS[name])


@pytest.mark.parametrize("name", sorted(ARGS))
def test_components_equal_scipy(name):
    v, tri = dirty(name)
    out = cleaned(name)
    rel, label = out["relabelled"], out["label"]
    live = np.flatnonzero(label >= 0)
    edges = cr.edge_faces(rel, label >= 0)
    rows, cols = [], []
    for faces in edges.values():
        rows += faces[:-1]
        cols += faces[1:]
    F = tri.shape[0]
    n, lab = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(F, F)), directed=False)
    assert np.unique(label[live]).size == np.unique(lab[live]).size == out["report"]["components"]
    for root in np.unique(label[live]):
        members = np.flatnonzero(label == root)
        assert members.min() == root and np.unique(lab[members]).size == 1


@pytest.mark.parametrize("name", sorted(ARGS))
def test_the_cleaned_mesh_is_manifold_and_the_maps_are_consistent(name):
    v, tri = dirty(name)
    out = cleaned(name)
    v2, t2, vmap, fmap, report = out["vertices"], out["indices"], out["vertex_map"], out["face_map"], out["report"]
    print(name, report)
    assert t2.shape[0] > 0 and cr.edge_valences(t2).max() <= 2          # every edge has at most two faces
    assert set(cr.fans_per_vertex(t2).values()) == {1}                 # every vertex has one fan
    assert np.array_equal(np.unique(t2), np.arange(v2.shape[0]))       # every output vertex is referenced
    assert (np.diff(fmap) > 0).all() and fmap.min() >= 0 and fmap.max() < tri.shape[0]
    rows = {p.tobytes() for p in v}
    assert all(p.tobytes() in rows for p in v2)                        # every output position is bitwise an input position
    # an output face is its input face, welded: position by position, up to the copies of split vertices
    assert np.array_equal(v2[t2], v[out["target"][tri[fmap]]])
    kept = vmap >= 0
    assert np.array_equal(v2[vmap[kept]], v[out["target"][kept]])
    originals = v2.shape[0] - report["vertices_split"]
    assert vmap.max() < originals and np.unique(vmap[kept]).size == originals
    assert report["edge_faces_removed"] >= report["edge_rounds"] >= 0
    assert tri.shape[0] - t2.shape[0] == (report["null_faces"] + report["duplicate_faces"] + report["component_faces_removed"]
                                          + report["edge_faces_removed"])


def test_what_the_junk_costs():
    for name in ("sheet", "tube"):
        r = cleaned(name)["report"]
        assert r["unreferenced"] >= 1 and r["merged"] >= 4 and r["null_faces"] >= 1 and r["duplicate_faces"] >= 6
        assert r["components_removed"] >= 2 and r["edge_faces_removed"] >= 1 and r["vertices_split"] >= 1
    assert cleaned("book4")["report"]["edge_rounds"] == 2 and cleaned("book6")["report"]["edge_rounds"] == 4
    assert cleaned("book4")["face_map"].tolist() == [0, 2]
    assert cleaned("cones")["report"]["vertices_split"] == 1
    heavy = cleaned("cloth_heavy")["report"]
    assert heavy["merged"] > 20 and heavy["null_faces"] > 0 and heavy["duplicate_faces"] > 0


def test_the_edge_rounds_are_neither_a_one_shot_rule_nor_in_place():
    """the two cases of tests/test_mesh_clean_gpu.py, on the statement alone"""
    v, tri = cr.two_edges((1.0, 2.0, 4.0), (2.0, -3.0))
    akey = cr.null_faces(v, tri)[1]
    ones = np.ones(tri.shape[0], dtype=bool)
    alive, rounds = cr.edge_rounds(tri, ones, akey)
    assert akey.tolist() == [9.0, 1.0, 4.0, 16.0, 36.0, 81.0] and rounds == 1
    assert alive.tolist() == [False, False, True, True, True, True]
    assert cr.one_shot_edge_rule(tri, ones, akey).tolist() == [False, False, False, True, True, True]
    v, tri = cr.two_edges((4.0, -5.0), (0.5, 2.0))
    akey = cr.null_faces(v, tri)[1]
    ones = np.ones(tri.shape[0], dtype=bool)
    alive, rounds = cr.edge_rounds(tri, ones, akey)
    assert akey.tolist() == [9.0, 16.0, 25.0, 2.25, 36.0] and rounds == 1
    assert alive.tolist() == [False, True, True, False, True]
    assert cr.in_place_edge_round(tri, ones, akey).tolist() == [False, True, True, True, True]
    assert cr.edge_valences(tri[alive]).max() <= 2


def test_cleaning_twice_changes_nothing():
    for name in ("sheet", "cones", "book6"):
        out = cleaned(name)
        again = cr.clean(out["vertices"], out["indices"], **ARGS[name])
        assert np.array_equal(again["vertices"], out["vertices"]) and np.array_equal(again["indices"], out["indices"])


def test_argument_errors_of_the_statement():
    v, tri = rr.cloth(3)
    with pytest.raises(ValueError, match="out of range"):
        cr.clean(v, np.array([[0, 1, v.shape[0]]]))
    bad = np.concatenate((v, [[0, 0, np.inf]])).astype(np.float32)
    cr.clean(bad, tri)                                                  # on a vertex no face names: fine
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        cr.clean(bad, tri)
    empty = cr.clean(v, tri[:0])
    assert empty["indices"].shape == (0, 3) and empty["report"]["unreferenced"] == v.shape[0]


# ---- the package, without a GPU -----------------------------------------------------------------------------------------------

def test_cpu_tensors_are_refused():
    from garmentdreamer_amd import mesh_clean as mc
    v, tri = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for call in (mc.clean_mesh, mc.merge_close_vertices, mc.remove_null_faces, mc.remove_duplicate_faces, mc.face_components,
                 mc.remove_small_components, mc.repair_non_manifold_edges, mc.split_non_manifold_vertices):
        with pytest.raises(ValueError, match=f"mesh_clean.{call.__name__}: the HIP kernels have no CPU path"):
            call(v, tri)


def test_the_bindings_cover_the_header():
    from garmentdreamer_amd import _native
    from garmentdreamer_amd.texture_field import NeTFRenderer
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gd_mesh_clean.h")).read()
    declared = set(re.findall(r"^int (gd_mesh_clean_\w+)\(", header, flags=re.M))
    assert declared == set(_native.MESH_CLEAN_SIGNATURES) and len(declared) == 17
    L = _native.lib()
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_mesh_clean.h but not exported"
        assert _native.error_channel(name) == "gd_mesh_last_error"
        count = len(re.search(name + r"\((.*?)\);", header, flags=re.S).group(1).split(","))
        assert count == len(_native.MESH_CLEAN_SIGNATURES[name][1]), name
    for macro, value in re.findall(r"^#define GD_MESH_CLEAN_STAT_(\w+) (\d+)", header, flags=re.M):
        assert getattr(_native, "CLEAN_STAT_" + macro) == int(value)
    assert int(re.search(r"#define GD_MESH_CLEAN_STATS (\d+)", header).group(1)) == _native.CLEAN_STATS
    assert int(re.search(r"#define GD_MESH_CLEAN_MAX_ROUNDS (\d+)", header).group(1)) == _native.CLEAN_MAX_ROUNDS
    # every entry validates before any device work: a bad call fails without a device
    assert L.gd_mesh_clean_check(None, 0, 0, None, None, None, None, None, None) == -1 and b"clean check" in L.gd_mesh_last_error()
    assert L.gd_mesh_clean_edge_table(None, 4, None, None, None, None) == -1 and b"clean edge table" in L.gd_mesh_last_error()
    assert L.gd_mesh_clean_fan_ranks(None, 3, 4, None, None) == -1 and b"clean fan ranks" in L.gd_mesh_last_error()
    one = (C.c_int32 * 4)()                                             # an aliased pair is named as such
    p = C.cast(one, C.c_void_p)
    assert L.gd_mesh_clean_edge_rounds(None, 1, p, p, p, 2, p, p, p) == -1 and b"distinct" in L.gd_mesh_last_error()
    assert L.gd_mesh_clean_duplicates(None, 1, p, p, p, p, p, p, p) == -1 and b"distinct" in L.gd_mesh_last_error()
    assert hasattr(NeTFRenderer, "from_mesh")
