"""GPU checks of the chart-based UV atlas (csrc/raster_atlas.hip, garmentdreamer_amd/texture_atlas.py) against the CPU
statement of its definition (tests/atlas_reference.py): every stage of every round by equality, each raw call into an
output buffer full of garbage; the whole ``chart_atlas``; the atlas through the package's own rasterizer, the bake and the
export."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import atlas_reference as ar
from tests import bake_reference as bref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GARBAGE = 0x5A5A5A5A
CASES = sorted(ar.PACKED)


def _ta():
    from garmentdreamer_amd import texture_atlas
    return texture_atlas


def _dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _junk(shape, dtype=torch.int32):
    return torch.full(shape, GARBAGE, dtype=torch.int32, device=DEV).view(dtype) if dtype != torch.int64 else \
        torch.full(shape, GARBAGE * (1 << 32) + GARBAGE, dtype=torch.int64, device=DEV)


def _same(t, want):
    got = t.cpu().numpy()
    want = np.asarray(want)
    if got.dtype == np.float32:
        return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
    return got.shape == want.shape and np.array_equal(got, want.astype(got.dtype))


def _raw_classes(v, tri):
    from garmentdreamer_amd._launch import launch
    cls = _junk((tri.shape[0],))
    launch("gd_atlas_face_class", DEV, v.shape[0], tri.shape[0], _dv(v), _dv(tri), cls)
    return cls


@pytest.mark.parametrize("make", [ar.tube, ar.cube, ar.helicoid, ar.ties, ar.with_degenerate, ar.single, ar.two_squares],
                         ids=lambda m: m.__name__)
def test_face_classes(make):
    v, tri = make()
    want = ar.face_class(v, tri)
    assert _same(_raw_classes(v, tri), want)
    assert _same(_ta().face_classes(_dv(v), _dv(tri.astype(np.int64))), want)
    if make is ar.ties:
        assert want.tolist() == [0, 1, 2, 0, 0]
    if make is ar.with_degenerate:
        assert want.tolist() == [4, 4, 6, 4, 4, 6]


def _raw_labels(conn, cls, layer, single):
    """hook + jump until nothing changes, by hand; (labels, sweeps)"""
    from garmentdreamer_amd import _native
    from garmentdreamer_amd._launch import launch
    parent = torch.arange(conn.F, dtype=torch.int32, device=DEV)
    for sweep in range(_native.ATLAS_MAX_SWEEPS):
        changed = torch.zeros(1, dtype=torch.int32, device=DEV)
        launch("gd_atlas_hook", DEV, conn.F, conn.E, conn.eh, cls, layer, single, parent, changed)
        launch("gd_atlas_jump", DEV, conn.F, parent)
        if not int(changed):
            return parent, sweep + 1
    raise AssertionError("the sweeps did not end")


def test_labels_of_the_strip_stay_within_the_sweep_bound():
    from garmentdreamer_amd import _native
    from garmentdreamer_amd.mesh_remesh import build_connectivity
    v, tri = ar.strip()
    conn = build_connectivity(_dv(tri), v.shape[0])
    cls = _raw_classes(v, tri)
    zero = torch.zeros(conn.F, dtype=torch.int32, device=DEV)
    labels, sweeps = _ta().chart_labels(conn, cls, return_sweeps=True)
    raw, raw_sweeps = _raw_labels(conn, cls, zero, zero)
    print(f"strip of {conn.F} faces: {sweeps} sweeps (by hand {raw_sweeps}), bound {_native.ATLAS_MAX_SWEEPS}")
    assert conn.F == 4096 and sweeps <= _native.ATLAS_MAX_SWEEPS
    assert not labels.any() and torch.equal(raw, labels)
    # ... and cut into pieces by layers and single faces
    rng = np.random.RandomState(2)
    layer = (np.arange(conn.F) // 300 % 2).astype(np.int32)
    single = (rng.uniform(size=conn.F) < 0.01).astype(np.int32)
    from tests import remesh_reference as rr
    want = ar.chart_labels(rr.Connectivity(tri, v.shape[0]), ar.face_class(v, tri), layer, single)
    assert len(set(want.tolist())) > 20
    assert _same(_ta().chart_labels(conn, cls, _dv(layer), _dv(single)), want)


@pytest.mark.parametrize("name", CASES)
def test_every_stage_of_every_round(name):
    """the rounds driven by hand, entry by entry, each output buffer full of garbage before the call"""
    from garmentdreamer_amd._launch import launch
    from garmentdreamer_amd.mesh_remesh import _scan, build_connectivity
    ta = _ta()
    v, tri, res, gutter, want = ar.packed(name)
    F, V = tri.shape[0], v.shape[0]
    dv, dt = _dv(v), _dv(tri)
    conn = build_connectivity(dt, V)
    cls = _raw_classes(v, tri)
    assert _same(cls, want["cls"])
    layer = torch.zeros(F, dtype=torch.int32, device=DEV)
    single = torch.zeros(F, dtype=torch.int32, device=DEV)
    for rnd, step in enumerate(want["trace"], start=1):
        assert _same(layer, step["layer"]) and _same(single, step["single"])
        labels, sweeps = _raw_labels(conn, cls, layer, single)
        assert _same(labels, step["labels"]), (name, rnd, sweeps)
        is_root = _junk((F,))
        launch("gd_atlas_roots", DEV, F, cls, labels, is_root)
        scan = _scan(is_root)
        C = int(scan[-1])
        assert C == step["bounds"].shape[0]
        face_chart, keys, bounds, count = _junk((F,)), _junk((C, 4)), _junk((C, 4), torch.float32), _junk((C,))
        launch("gd_atlas_bounds", DEV, V, F, C, dv, dt, cls, labels, scan, face_chart, keys, bounds, count)
        assert _same(face_chart, step["face_chart"]) and _same(bounds, step["bounds"]) and _same(count, step["count"])
        scale, offsets, sizes = ta.pack_charts(bounds.cpu().numpy(), res, gutter)
        assert scale == step["scale"] and np.array_equal(offsets, step["offsets"]) and np.array_equal(sizes, step["sizes"])
        corner_xy, key = _junk((F, 3, 2)), _junk((3 * F,), torch.int64)
        launch("gd_atlas_emit", DEV, V, F, C, res, gutter, float(scale), dv, dt, cls, face_chart, bounds, _dv(offsets),
               corner_xy, key)
        assert _same(corner_xy, step["corner_xy"]), (name, rnd)
        rows, inverse = torch.unique(key, sorted=True, return_inverse=True)
        T = rows.shape[0]
        vt, ft = _junk((T, 2), torch.float32), _junk((F, 3))
        launch("gd_atlas_write_vt", DEV, 3 * F, T, res, inverse.contiguous(), corner_xy, vt, ft)
        assert _same(vt, step["vt"]) and _same(ft, step["ft"]), (name, rnd)
        rast = ta._rasterize_atlas(vt, ft, res)
        lost = _junk((F,))
        launch("gd_atlas_lost_faces", DEV, F, res, res, corner_xy, rast, int(rnd >= 8), lost, layer, single)
        assert _same(lost, step["lost"]), (name, rnd, int(lost.sum()), int(step["lost"].sum()))
    assert not lost.any()


@functools.lru_cache(maxsize=None)
def _atlas(name, max_rounds=8):
    """chart_atlas of a PACKED case with its trace; shared, read-only"""
    v, tri, res, gutter, _ = ar.packed(name)
    trace = []
    vt, ft, info = _ta().chart_atlas(_dv(v), _dv(tri), res, gutter, max_rounds, trace=trace)
    return vt, ft, info, trace


@pytest.mark.parametrize("name", CASES)
def test_chart_atlas_equals_the_statement_and_itself(name):
    v, tri, res, gutter, want = ar.packed(name)
    vt, ft, info, trace = _atlas(name)
    assert vt.is_cuda and vt.dtype == torch.float32 and ft.is_cuda and ft.dtype == torch.int32
    assert _same(vt, want["vt"]) and _same(ft, want["ft"]) and _same(info["face_chart"], want["face_chart"])
    assert info["face_chart"].is_cuda and info["face_chart"].dtype == torch.int32
    for k in ("num_charts", "scale", "rounds", "lost_per_round", "singletons", "seam_edges", "coverage"):
        assert info[k] == want[k], k
    assert len(trace) == len(want["trace"])
    print(name, "sweeps per round", [got["sweeps"] for got in trace], "lost per round", info["lost_per_round"])
    for got, step in zip(trace, want["trace"]):
        for k in ("layer", "single", "labels", "face_chart", "bounds", "count", "corner_xy", "vt", "ft", "lost"):
            assert _same(got[k], step[k]), k
    vt2, ft2, info2 = _ta().chart_atlas(_dv(v), _dv(tri.astype(np.int64)), res, gutter)          # again, int64 indices
    assert torch.equal(vt2.view(torch.int32), vt.view(torch.int32)) and torch.equal(ft2, ft)
    assert torch.equal(info2["face_chart"], info["face_chart"])
    assert {k: x for k, x in info2.items() if k != "face_chart"} == {k: x for k, x in info.items() if k != "face_chart"}


def test_the_helicoid_with_one_round_makes_singletons():
    v, tri, res, gutter, _ = ar.packed("helicoid")
    want = ar.chart_atlas(v, tri, res, gutter, max_rounds=1)
    vt, ft, info, trace = _atlas("helicoid", 1)
    assert info["singletons"] == want["singletons"] > 0 and info["lost_per_round"] == want["lost_per_round"]
    assert info["num_charts"] == want["num_charts"] and _same(vt, want["vt"]) and _same(ft, want["ft"])
    assert _same(trace[-1]["single"], want["trace"][-1]["single"])


@pytest.mark.parametrize("name", CASES)
def test_p1_through_the_packages_rasterizer(name):
    v, tri, res, gutter, want = ar.packed(name)
    vt, ft, info, _ = _atlas(name)
    rast = _ta()._rasterize_atlas(vt, ft, res)
    owner = rast[..., 3].cpu().numpy().astype(np.int64) - 1
    assert np.array_equal(owner >= 0, bref.chart_coverage(vt.cpu().numpy(), ft.cpu().numpy(), res, res))
    own = np.full((res, res), -1, dtype=np.int64)                       # per face, its own coverage
    xy = want["corner_xy"]
    for f in range(tri.shape[0]):
        r, c = ar.face_cover(xy[f], res, res)
        assert (own[r, c] == -1).all()                                  # nobody else's
        own[r, c] = f
    assert np.array_equal(owner, own)                                   # every covered texel lies in its owner's coverage


def test_bake_on_the_chart_atlas_of_the_tube():
    from garmentdreamer_amd import mesh_render as mr
    from garmentdreamer_amd import texture_bake as tb
    from tests.test_texture_bake_gpu import PAD, RES, _baked
    q = _baked()
    v, tri, res, gutter, want = ar.packed("tube")
    assert res == RES and np.array_equal(tri, q["tri"])
    vt, ft, info, _ = _atlas("tube")
    assert vt.shape[0] < 3 * tri.shape[0] and vt.shape[0] == 4 * 7 * 13          # 7 columns of vertices per chart
    out = tb.bake_texture(q["field"], _dv(v), _dv(tri), vt, ft, resolution=RES, padding=PAD)
    cover = bref.chart_coverage(want["vt"], want["ft"], RES, RES)
    assert np.array_equal(out["mask"].cpu().numpy(), cover)
    pos = torch.cat((vt * 2.0 - 1.0, torch.zeros_like(vt[:, :1]), torch.ones_like(vt[:, :1])), dim=1).contiguous()
    xyz = mr.interpolate(_dv(v), mr.rasterize(pos, ft, (RES, RES)), _dv(tri))
    with torch.no_grad():
        direct = q["field"](xyz.view(-1, 3), out["mask"].view(-1)).view(RES, RES, 3).cpu().numpy()
    want8 = bref.resolve_u8(direct, np.arange(RES * RES, dtype=np.int32).reshape(RES, RES))
    got8 = out["albedo"].cpu().numpy()
    assert np.array_equal(got8[cover], want8[cover]) and len(np.unique(got8[cover])) > 20
    grid_vt, grid_ft = tb.grid_atlas(tri.shape[0], RES, gutter=gutter)
    grid = bref.chart_coverage(grid_vt, grid_ft, RES, RES).mean()
    print(f"tube at {RES}^2, gutter {gutter}: chart atlas covers {info['coverage']:.4f} of the texel centres in "
          f"{info['num_charts']} charts with {info['seam_edges']} seam edges and {vt.shape[0]} vt rows; grid_atlas covers "
          f"{grid:.4f} with {grid_vt.shape[0]} rows")
    assert info["coverage"] == want["coverage"] == cover.mean()


def _export(tmp_path, name, **kw):
    from garmentdreamer_amd import texture_field as tf
    from tests.test_texture_bake_gpu import PAD, RES, _baked
    q = _baked()
    renderer = tf.NeTFRenderer(_dv(q["v"]), _dv(q["tri"]), _dv(q["vn"]), q["field"])
    path = str(tmp_path / name / "mesh.obj")
    written = renderer.export_mesh(path, texture_resolution=RES, padding=PAD, **kw)
    stem = os.path.splitext(path)[0]
    assert written == [path, stem + ".mtl", stem + "_albedo.png"] and all(os.path.isfile(p) for p in written)
    return written


def test_export_mesh_with_the_chart_atlas(tmp_path):
    from PIL import Image
    from garmentdreamer_amd import texture_bake as tb
    from tests.test_texture_bake_gpu import PAD, RES, _baked
    q = _baked()
    written = _export(tmp_path, "chart", atlas="chart")
    v2, f2, vt2, ft2 = tb.load_obj_uv(written[0])
    F = q["tri"].shape[0]
    assert np.array_equal(f2, q["tri"].astype(np.int64)) and np.array_equal(v2, q["v"].astype(np.float64))
    want_vt, want_ft, _ = _ta().chart_atlas(_dv(q["v"]), _dv(q["tri"]), RES)            # export's defaults: gutter 2
    assert np.array_equal(ft2, want_ft.cpu().numpy().astype(np.int64)) and ft2.shape == (F, 3)
    assert vt2.shape[0] == want_vt.shape[0] < 3 * F and len(np.unique(ft2)) == vt2.shape[0]      # shared rows, all used
    assert np.array_equal(vt2[:, 0], want_vt[:, 0].cpu().numpy().astype(np.float64))
    baked = tb.bake_texture(q["field"], _dv(q["v"]), _dv(q["tri"]), want_vt, want_ft, resolution=RES, padding=PAD)
    assert np.array_equal(np.asarray(Image.open(written[2])), baked["albedo"].cpu().numpy())
    # the caller's UVs still win
    mine = _export(tmp_path, "mine", atlas="chart", vt=q["vt"], ft=q["ft"])
    default = _export(tmp_path, "default")
    grid = _export(tmp_path, "grid", atlas="grid")
    for a, b, c in zip(default, grid, mine):
        assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    assert open(default[0], "rb").read() != open(written[0], "rb").read()
    with pytest.raises(ValueError, match="atlas must be"):
        _export(tmp_path, "bad", atlas="x")


def test_refusals():
    ta = _ta()
    v, tri = ar.fan()
    with pytest.raises(ValueError, match="non-manifold"):
        ta.chart_atlas(_dv(v), _dv(tri), 64)
    v, tri = ar.cube()
    with pytest.raises(ValueError, match="too small"):
        ta.chart_atlas(_dv(v), _dv(tri), 8, gutter=2)
    with pytest.raises(ValueError, match="resolution must be"):
        ta.chart_atlas(_dv(v), _dv(tri), 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ta.chart_atlas(torch.from_numpy(v), _dv(tri))
