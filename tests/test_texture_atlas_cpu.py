"""The statement of the chart-based UV atlas (tests/atlas_reference.py, include/gd_atlas.h) on the CPU: the properties an
atlas must have (injective at texel centres, gutters, bounded stretch, orientation), the chart counts of known meshes, the
overlap peeling on a helicoid, the packer; and what of garmentdreamer_amd/texture_atlas.py needs no GPU: its packer
against the statement's, the bindings, the argument checks of every entry."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import atlas_reference as ar
from tests import bake_reference as bref
from tests import remesh_reference as rr

CASES = sorted(ar.PACKED)


def _area3d(v, tri):
    p = v.astype(np.float64)
    return 0.5 * np.linalg.norm(np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]]), axis=1)


@pytest.mark.parametrize("name", CASES)
def test_p1_injective_at_texel_centres(name):
    v, tri, res, gutter, out = ar.packed(name)
    assert out["times"].max() == 1                                  # no centre is covered by two faces
    assert not out["trace"][-1]["lost"].any()
    for f in range(tri.shape[0]):                                   # ... said per face: what it covers it owns
        r, c = ar.face_cover(out["corner_xy"][f], res, res)
        assert (out["owner"][r, c] == f).all()
    cover = bref.chart_coverage(out["vt"], out["ft"], res, res)     # the bake's own statement of coverage
    assert np.array_equal(cover, out["owner"] >= 0) and out["coverage"] == cover.mean()
    # the rasterizer's snapping of vt recovers the integer corners
    snapped = np.rint(((out["vt"] * np.float32(2) - np.float32(1)) * np.float32(0.5) + np.float32(0.5)) * np.float32(256 * res))
    assert snapped.dtype == np.float32 and np.array_equal(snapped[out["ft"]].astype(np.int32), out["corner_xy"])


@pytest.mark.parametrize("name", CASES)
def test_p2_gutters(name):
    v, tri, res, gutter, out = ar.packed(name)
    chart = np.where(out["owner"] >= 0, out["face_chart"][np.maximum(out["owner"], 0)], -1)
    reach = 2 * gutter - 1
    for dr in range(0, reach + 1):
        for dc in range(-reach, reach + 1):
            a = chart[dr:, max(dc, 0):res + min(dc, 0)]
            b = chart[:res - dr, max(-dc, 0):res + min(-dc, 0)]
            assert not ((a >= 0) & (b >= 0) & (a != b)).any(), (dr, dc)
    rects = [(x, y, x + w, y + h) for (x, y), (w, h) in zip(out["offsets"], out["rects"])]
    assert all(isinstance(t, int) for r in rects for t in r)
    assert all(0 <= x0 < x1 <= res and 0 <= y0 < y1 <= res for x0, y0, x1, y1 in rects)
    for i, p in enumerate(rects):
        for q in rects[i + 1:]:
            assert p[2] <= q[0] or q[2] <= p[0] or p[3] <= q[1] or q[3] <= p[1]
    # every chart's texels lie in the inner part of its rectangle
    for c, (x0, y0, x1, y1) in enumerate(rects):
        r, col = np.nonzero(chart == c)
        assert r.size and x0 + gutter <= col.min() and col.max() < x1 - gutter and y0 + gutter <= r.min() and r.max() < y1 - gutter


@pytest.mark.parametrize("name", CASES)
def test_p3_stretch_and_p4_orientation(name):
    """UV area (texels^2) over s^2 x the 3-D area is |n_k| / |n| of the face: at most 1, and at least 1 / sqrt(3) because k
    is the largest component.  The snapping moves every corner coordinate by at most d = 1/512 texel, plus the two fp32
    roundings of (a - a_min) s, each at most 2^-24 of a value below the resolution.  With edge vectors e1, e2 (whose
    components then move by at most 2 d) the doubled area e1 x e2 changes by at most 2 d (|e1|_1 + |e2|_1) + 8 d^2, taken
    here with the snapped edges lengthened by 2 d per component; 1e-6 covers the float32 scale and normals."""
    v, tri, res, gutter, out = ar.packed(name)
    xy = out["corner_xy"].astype(np.float64) / 256.0
    e1, e2 = xy[:, 1] - xy[:, 0], xy[:, 2] - xy[:, 0]
    area_uv = 0.5 * (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
    live = out["cls"] != ar.DEGENERATE
    assert (area_uv[live] > 0).all() and (area_uv[~live] == 0).all()                       # P4
    vt, ft = out["vt"].astype(np.float64), out["ft"]
    d1, d2 = vt[ft[:, 1]] - vt[ft[:, 0]], vt[ft[:, 2]] - vt[ft[:, 0]]
    assert ((d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0])[live] > 0).all()                   # ... in vt itself
    d = 1.0 / 512.0 + 2.0 * res * 2.0 ** -24
    l1 = np.abs(e1).sum(axis=1) + np.abs(e2).sum(axis=1) + 8 * d
    slack = 0.5 * (2 * d * l1 + 8 * d * d)
    s = out["scale"]
    area = _area3d(v, tri)
    ratio = area_uv[live] / (s * s * area[live])
    eps = slack[live] / (s * s * area[live]) + 1e-6
    print(f"{name}: scale {s:.4f}, stretch {ratio.min():.4f} .. {ratio.max():.4f}, largest eps {eps.max():.5f}")
    assert (ratio >= 1 / math.sqrt(3) - eps).all() and (ratio <= 1 + eps).all()


def test_chart_counts_labels_and_seams():
    for name, charts in (("cube", 6), ("tube", 4), ("two_squares", 2), ("with_degenerate", 2), ("single", 1)):
        v, tri, res, gutter, out = ar.packed(name)
        assert out["num_charts"] == charts and out["rounds"] == 1 and out["lost_per_round"] == [0], name
        labels = out["trace"][0]["labels"]
        conn = rr.Connectivity(tri, v.shape[0])
        # the labels are the lowest face index of a component, found here by flooding from every face
        for f in range(tri.shape[0]):
            seen, todo = {f}, [f]
            while todo:
                x = todo.pop()
                for e in conn.fe[3 * x:3 * x + 3]:
                    for h in conn.eh[e]:
                        y = h // 3
                        if h >= 0 and y not in seen and out["cls"][y] == out["cls"][x] != ar.DEGENERATE:
                            seen.add(y)
                            todo.append(y)
            assert labels[f] == min(seen)
        assert sorted(set(labels[out["cls"] != ar.DEGENERATE].tolist())) == \
            [int(np.flatnonzero(out["face_chart"] == c)[0]) for c in range(charts)]
        assert np.array_equal(np.bincount(out["face_chart"][out["face_chart"] >= 0]), out["trace"][0]["count"])
    assert ar.packed("tube")[4]["seam_edges"] == 4 * 12
    assert set(ar.packed("tube")[4]["cls"].tolist()) == {0, 1, 2, 3}
    assert sorted(set(ar.packed("cube")[4]["cls"].tolist())) == [0, 1, 2, 3, 4, 5] and ar.packed("cube")[4]["seam_edges"] == 12 * 4
    deg = ar.packed("with_degenerate")[4]
    assert deg["cls"].tolist() == [4, 4, 6, 4, 4, 6] and deg["face_chart"].tolist() == [0, 0, -1, 1, 1, -1]
    assert (deg["corner_xy"][[2, 5]] == 0).all() and len(set(deg["ft"][[2, 5]].ravel().tolist())) == 1


def test_welded_rows():
    for name in CASES:
        v, tri, res, gutter, out = ar.packed(name)
        ft, fc = out["ft"], out["face_chart"]
        assert out["vt"].shape[0] < 3 * tri.shape[0] or tri.shape[0] == 1
        owner_chart = {}
        for f in range(tri.shape[0]):
            for i in range(3):
                assert owner_chart.setdefault(int(ft[f, i]), int(fc[f])) == int(fc[f])          # no row in two charts
        pairs = {(int(fc[f]), int(tri[f, i])) for f in range(tri.shape[0]) for i in range(3) if fc[f] >= 0}
        assert out["vt"].shape[0] == len(pairs) + int((fc < 0).any())                          # one row per (chart, vertex)


def test_tie_classes():
    v, tri = ar.ties()
    assert ar.face_normals(v, tri).tolist() == [[1, 1, 0], [-1, -1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1]]
    assert ar.face_class(v, tri).tolist() == [0, 1, 2, 0, 0]


def test_the_strip_is_one_chart():
    v, tri = ar.strip()
    conn = rr.Connectivity(tri, v.shape[0])
    assert tri.shape[0] == 4096 and not ar.chart_labels(conn, ar.face_class(v, tri)).any()


def test_the_helicoid_is_peeled():
    v, tri, res, gutter, out = ar.packed("helicoid")
    assert tri.shape[0] == 384 and set(out["cls"].tolist()) == {4}
    assert len(set(out["trace"][0]["labels"].tolist())) == 1                 # one component, which lies over itself
    print("helicoid: lost per round", out["lost_per_round"], "charts", out["num_charts"], "singletons", out["singletons"])
    assert out["lost_per_round"][0] > 0 and out["lost_per_round"][-1] == 0
    assert 1 < out["rounds"] <= 8
    assert out["singletons"] <= tri.shape[0] // 2
    assert out["num_charts"] <= 8                                            # sheets, not confetti
    # a tight max_rounds turns what is still lost into charts of their own, and still ends injective
    tight = ar.chart_atlas(v, tri, res, gutter, max_rounds=1)
    assert tight["singletons"] == out["lost_per_round"][0] and tight["times"].max() == 1
    single_faces = np.flatnonzero(tight["trace"][-1]["single"])
    assert np.array_equal(tight["trace"][-1]["labels"][single_faces], single_faces)


def test_non_manifold_and_small_resolutions_are_refused():
    v, tri = ar.fan()
    with pytest.raises(ValueError, match="non-manifold"):
        ar.chart_atlas(v, tri, 64)
    v, tri = ar.cube()
    with pytest.raises(ValueError, match="too small"):
        ar.chart_atlas(v, tri, 8, gutter=2)                                 # six charts of 5 x 5 at least


# ---- the package, without a GPU -----------------------------------------------------------------------------------------------

def test_the_packer_is_deterministic_and_equals_the_statements():
    from garmentdreamer_amd import texture_atlas as ta
    rng = np.random.RandomState(5)
    sets = [ar.packed(name)[4]["trace"][0]["bounds"] for name in CASES]
    lo = rng.uniform(-1, 1, (40, 2)).astype(np.float32)
    sets.append(np.concatenate((lo, lo + rng.uniform(0.01, 0.6, (40, 2)).astype(np.float32)), axis=1))
    for bounds in sets:
        for res, gutter in ((256, 2), (128, 1), (97, 0)):
            try:
                want = ar.pack(bounds, res, gutter)
            except ValueError:
                with pytest.raises(ValueError, match="too small"):
                    ta.pack_charts(bounds, res, gutter)
                continue
            s, off, sizes = ta.pack_charts(bounds, res, gutter)
            s2, off2, sizes2 = ta.pack_charts(bounds.copy(), res, gutter)
            assert s.dtype == np.float32 and off.dtype == np.int32 and sizes.dtype == np.int32
            assert s == s2 and np.array_equal(off, off2) and np.array_equal(sizes, sizes2)
            assert s == want[0] and off.tolist() == [list(t) for t in want[1]] and sizes.tolist() == [list(t) for t in want[2]]
    with pytest.raises(ValueError, match="too small"):
        ta.pack_charts(sets[CASES.index("cube")], 8, 2)


def test_the_bindings_cover_the_header():
    from garmentdreamer_amd import _native
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gd_atlas.h")).read()
    declared = sorted(re.findall(r"^int (gd_atlas_\w+)\(", header, flags=re.M))
    assert declared == sorted(_native.ATLAS_SIGNATURES) and len(declared) == 8
    L = _native.lib()
    others = [getattr(_native, n) for n in dir(_native) if n.endswith("SIGNATURES") and n != "ATLAS_SIGNATURES"]
    assert len(others) >= 13
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_atlas.h but not exported"
        assert _native.error_channel(name) == "gd_mesh_last_error"
        assert not any(name in table for table in others)
        count = len(re.search(name + r"\((.*?)\);", header, flags=re.S).group(1).split(","))
        assert count == len(_native.ATLAS_SIGNATURES[name][1]), name
    for macro, value in (("DEGENERATE", _native.ATLAS_DEGENERATE), ("MAX_SWEEPS", _native.ATLAS_MAX_SWEEPS),
                         ("MAX_RESOLUTION", _native.ATLAS_MAX_RESOLUTION), ("MAX_GUTTER", _native.ATLAS_MAX_GUTTER),
                         ("BISECTION_STEPS", _native.ATLAS_BISECTION_STEPS)):
        assert int(re.search(rf"#define GD_ATLAS_{macro} (\d+)", header).group(1)) == value
    assert ar.DEGENERATE == _native.ATLAS_DEGENERATE and ar.BISECTION_STEPS == _native.ATLAS_BISECTION_STEPS


def test_the_source_is_built_without_contraction():
    from garmentdreamer_amd import _build
    assert ("raster_atlas.hip", ["-ffp-contract=off"]) in _build.RASTER_SOURCES


X = 0x1000            # non-null and never followed: every call below is refused before any device work
# entry -> (a valid argument list after the stream, the positions of its pointers, {position: a bad size})
ENTRIES = {
    "gd_atlas_face_class": ([3, 1, X, X, X], (2, 3, 4), {0: 0, 1: 0}),
    "gd_atlas_hook": ([1, 3, X, X, X, X, X, X], (2, 3, 4, 5, 6, 7), {0: 0, 1: 0}),
    "gd_atlas_jump": ([1, X], (1,), {0: 0}),
    "gd_atlas_roots": ([1, X, X, X], (1, 2, 3), {0: 1 << 29}),
    "gd_atlas_bounds": ([3, 1, 1, X, X, X, X, X, X, X, X, X], tuple(range(3, 12)), {0: 0, 1: 0, 2: 0}),
    "gd_atlas_emit": ([3, 1, 1, 64, 2, 1.0, X, X, X, X, X, X, X, X], tuple(range(6, 14)),
                      {0: 0, 1: 0, 2: 2, 3: 0, 4: 65, 5: 0.0}),
    "gd_atlas_write_vt": ([3, 3, 64, X, X, X, X], (3, 4, 5, 6), {0: 4, 1: 4, 2: 1 << 20}),
    "gd_atlas_lost_faces": ([1, 8, 8, X, X, 0, X, X, X], (3, 4, 6, 7, 8), {0: 0, 1: 0, 2: 1 << 20}),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_bad_calls_return_minus_one_with_a_message(name):
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert sorted(ENTRIES) == sorted(_native.ATLAS_SIGNATURES)
    good, pointers, sizes = ENTRIES[name]
    assert len(good) + 1 == len(_native.ATLAS_SIGNATURES[name][1])
    assert set(pointers) == {i for i, a in enumerate(_native.ATLAS_SIGNATURES[name][1][1:]) if a is _native._vp}
    spoil = [(i, None, "null pointer") for i in pointers] + [(i, bad, "must") for i, bad in sizes.items()]
    for i, bad, piece in spoil:
        args = list(good)
        args[i] = bad
        L.gd_mesh_rasterize(None, 3, 1, 0, 8, None, None, None, None)          # another text in the channel first
        assert getattr(L, name)(None, *args) == -1, (name, i)
        text = L.gd_mesh_last_error().decode()
        assert text.startswith("atlas ") and piece in text, (name, i, text)
        with pytest.raises(RuntimeError, match=name):
            _native.checked(name, -1)


def test_cpu_tensors_and_bad_arguments_are_refused():
    from garmentdreamer_amd import texture_atlas as ta
    from garmentdreamer_amd import texture_bake as tb
    v, tri = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for call in (lambda: ta.chart_atlas(v, tri), lambda: ta.face_classes(v, tri)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match="atlas must be"):
        tb.export_textured_mesh("unused.obj", None, v, tri, atlas="x")
