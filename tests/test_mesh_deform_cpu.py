"""CPU-side checks of the position gradients of the mesh render path.  They pin the REFERENCE (tests/mesh_grad_reference.py)
so that it and the kernels cannot share a convention error: its continuous functions agree with the snapped forward of
tests/mesh_reference.py to within what snapping can move, its autograd gradients agree with finite differences, and the
gd_mesh_* entries of include/gd_mesh_deform.h are exported, bound and validate their arguments without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_grad_reference as gref
from tests import mesh_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 64
# A snapped coordinate is the unsnapped one rounded to 1/256 pixel: at most half a sub-pixel, 1/512, away, plus the fp32
# rounding of the snap's own arithmetic (three operations on values up to 256 W = 2^14 sub-pixels: well below 2^-14 pixel)
DELTA = 1.0 / 512 + 2.0 ** -14


def _big_scene():
    pos, tri = gref.big_triangle_scene(H, W)
    rast = ref.rasterize(pos, tri, H, W)
    return pos, tri, rast


def test_ideal_barycentrics_agree_with_the_snapped_forward():
    """Bound.  Let b_i be the screen-space barycentric of the unsnapped triangle T and b'_i that of the snapped T'.  Both
    are affine in the pixel; d = b'_i - b_i is affine too, and at a vertex v'_m of T' it is b'_i(v'_m) - b_i(v'_m)
    = b_i(v_m) - b_i(v'_m) = -grad(b_i) . (v'_m - v_m), where |grad b_i| = 1 / h_i (h_i: the altitude on edge i) and
    |v'_m - v_m| <= sqrt(2) DELTA.  A covered pixel centre is a convex combination of the v'_m, so
    |b'_i - b_i| <= eps = sqrt(2) DELTA / h_min on every covered pixel.  With p_i = b_i / w_i, s = sum p_i, u = p_0 / s:
    u - u' = (u' (s - s') - (p_0 - p'_0)) / s, |p_0 - p'_0| <= eps rw_max, |s - s'| <= 3 eps rw_max, |u'| <= 1 and
    s >= s' - |s - s'| >= rw_min - 3 eps rw_max, hence |u - u'| <= 4 eps rw_max / (rw_min - 3 eps rw_max); v likewise.
    1e-6 is added for the fp32 roundings of the snapped statement itself (a handful at 2^-24 on values <= 1)."""
    pos, tri, rast = _big_scene()
    ids = rast[..., 3].astype(np.int64)
    p64 = torch.from_numpy(pos).double()
    sx, sy = (a.numpy() for a in gref.screen_xy(p64, H, W))
    uv = gref.ideal_uv(p64, tri, ids).numpy()
    assert (ids > 0).sum() > 800
    for t, (i0, i1, i2) in enumerate(tri):
        x, y = sx[[i0, i1, i2]], sy[[i0, i1, i2]]
        edges = np.hypot(x - np.roll(x, -1), y - np.roll(y, -1))
        assert edges.min() >= 16.0                                      # the scene is what it claims to be
        area2 = abs((x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]))
        eps = np.sqrt(2.0) * DELTA / (area2 / edges.max())              # shortest altitude = 2 area / longest edge
        rw = 1.0 / pos[[i0, i1, i2], 3].astype(np.float64)
        bound = 4 * eps * rw.max() / (rw.min() - 3 * eps * rw.max()) + 1e-6
        mine = ids == t + 1
        assert mine.sum() > 100
        err = np.abs(uv[mine] - rast[mine][:, :2].astype(np.float64)).max()
        print("triangle", t, "max |ideal - snapped| (u, v)", err, "bound", bound)
        assert 0 < err <= bound
    assert not uv[ids == 0].any()


def test_ideal_antialias_weights_agree_with_the_snapped_analysis():
    """Bound.  x* = al_a + (al_b - al_a) s, s = (line - on_a) / D, D = on_b - on_a, from the snapped coordinates (where
    0 <= s <= 1: the edge straddles the line).  Moving the four coordinates by at most DELTA each gives
    s' - s = -(e3 (1 - s) + e4 s) / D', so |s' - s| <= DELTA / (|D| - 2 DELTA), and
    x*' - x* = e1 (1 - s') + e2 s' + (al_b - al_a) (s' - s), so
    |x*' - x*| <= DELTA (1 + 2 |s' - s|) + |al_b - al_a| DELTA / (|D| - 2 DELTA).  t = |x* - centre| and w = +-(t - 0.5)
    move by no more.  1e-5 (1 + slope) is added for the fp32 roundings of the snapped statement (coordinates up to 64)."""
    pos, tri, rast = _big_scene()
    opp = ref.build_opposite(tri)
    info = {}
    wts = ref.antialias_weights(rast, pos, tri, opp, info)
    assert min(info["to_outer"], info["to_inner"], info["horizontal"], info["vertical"], info["boundary"]) >= 5, info
    pairs = gref.antialias_pairs(rast, pos, tri, opp)
    ideal = gref.ideal_weights(torch.from_numpy(pos).double(), pairs, H, W).numpy()
    defined = np.zeros((H, W, 4), bool)
    defined[pairs["r"], pairs["c"], pairs["k"]] = True
    assert defined.sum() == len(pairs["r"]) >= (wts != 0).sum() >= 50
    assert not wts[~defined].any() and not ideal[~defined].any()       # the re-derived decisions are the analysis's own
    _, X, Y, _, _ = ref.snap_vertices(pos, H, W)
    hor = pairs["horizontal"].astype(bool)
    a, b = pairs["a"], pairs["b"]
    d_on = np.abs(np.where(hor, Y[b] - Y[a], X[b] - X[a])) / 256.0
    d_al = np.abs(np.where(hor, X[b] - X[a], Y[b] - Y[a])) / 256.0
    assert d_on.min() > 1.0
    ds = DELTA / (d_on - 2 * DELTA)
    bound = DELTA * (1 + 2 * ds) + d_al * ds + 1e-5 * (1 + d_al / d_on)
    err = np.abs(ideal[pairs["r"], pairs["c"], pairs["k"]] - wts[pairs["r"], pairs["c"], pairs["k"]].astype(np.float64))
    print("max |ideal - snapped| weight", err.max(), "largest bound", bound.max(), "worst ratio", (err / bound).max())
    assert err.max() > 0 and np.all(err <= bound)


def _central_differences(fn, pos, h):
    g = np.zeros(pos.shape)
    for v in range(pos.shape[0]):
        for j in range(4):
            lo, hi = pos.copy(), pos.copy()
            lo[v, j] -= h
            hi[v, j] += h
            g[v, j] = (fn(hi) - fn(lo)) / (2 * h)
    return g


def test_autograd_gradients_agree_with_central_differences():
    pos, tri, rast = _big_scene()
    ids = rast[..., 3].astype(np.int64)
    opp = ref.build_opposite(tri)
    pairs = gref.antialias_pairs(rast, pos, tri, opp)
    wts = ref.antialias_weights(rast, pos, tri, opp)
    rng = np.random.RandomState(0)
    attr = rng.uniform(-1, 1, size=(pos.shape[0], 3))
    dout = rng.uniform(-1, 1, size=(H, W, 3))
    color = rng.uniform(0, 1, size=(H, W, 3))
    p64 = pos.astype(np.float64)
    t = torch.from_numpy

    def interp_loss(p):
        out = gref.interpolate(t(attr), gref.ideal_uv(t(p), tri, ids), ids, tri)
        return float((out * t(dout)).sum())

    def aa_loss(p):
        return float((gref.antialias_apply(t(color), gref.ideal_weights(t(p), pairs, H, W)) * t(dout)).sum())

    # 1e-6 steps of quantities of order 1 in float64: truncation ~1e-12, rounding ~1e-16 * |L| / 1e-6 ~ 1e-8
    for name, fn, grad in (("interpolate o rasterize", interp_loss,
                            gref.grad_interpolate_rasterize(p64, tri, rast, attr, dout)),
                           ("antialias", aa_loss, gref.grad_antialias(p64, pairs, wts, color, dout))):
        fd = _central_differences(fn, p64, 1e-6)
        err = np.abs(fd - grad).max() / np.abs(grad).max()
        print(name, "max |fd - autograd| / max |autograd|", err)
        assert np.abs(grad).max() > 0 and err <= 1e-6
        assert not grad[:, 2].any() and not fd[:, 2].any()              # z receives nothing
        assert np.abs(grad[:, 3]).max() > 0                             # w does


def test_deform_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gd_mesh_deform.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gd_mesh_[a-z0-9_]+)\s*\(", text)))
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert len(declared) == 6
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_mesh_deform.h but not exported"
    assert sorted(_native.MESH_DEFORM_SIGNATURES) == declared
    # scratch: the [F][3][4] corner slab
    assert L.gd_mesh_rasterize_backward_scratch_bytes(1000) >= 1000 * 12 * 4
    assert L.gd_mesh_antialias_backward_pos_scratch_bytes(1000) >= 1000 * 12 * 4
    assert L.gd_mesh_rasterize_backward_scratch_bytes(-1) == 0
    # argument validation before any device work
    assert L.gd_mesh_interpolate_backward_rast(None, 3, 1, 9, 8, 8, *([None] * 5)) == -1
    assert b"[1, 8]" in L.gd_mesh_last_error()
    assert L.gd_mesh_interpolate_backward_rast(None, 3, 1, 3, 8, 8, *([None] * 5)) == -1 and b"null" in L.gd_mesh_last_error()
    assert L.gd_mesh_rasterize_backward(None, 3, 1, 0, 8, *([None] * 8)) == -1 and b"positive" in L.gd_mesh_last_error()
    assert L.gd_mesh_rasterize_backward(None, 3, 1, 8, 8, *([None] * 8)) == -1 and b"null" in L.gd_mesh_last_error()
    assert L.gd_mesh_antialias_backward_pos(None, 3, 1, 0, 8, 8, *([None] * 10)) == -1
    assert L.gd_mesh_antialias_backward_pos(None, 3, 1, 3, 8, 8, *([None] * 10)) == -1 and b"null" in L.gd_mesh_last_error()
    assert L.gd_mesh_visible_vertices(None, 3, 1, 0, None, None, None) == -1
    assert L.gd_mesh_visible_vertices(None, 3, 1, 64, None, None, None) == -1 and b"null" in L.gd_mesh_last_error()


def test_ops_reject_cpu_tensors():
    from garmentdreamer_amd import mesh_deform as md
    pos, tri = torch.zeros(3, 4, requires_grad=True), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        md.rasterize(pos, tri, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        md.interpolate(torch.zeros(3, 3), torch.zeros(8, 8, 4), tri, pos)
    with pytest.raises(RuntimeError, match="no CPU path"):
        md.antialias(torch.zeros(8, 8, 3), torch.zeros(8, 8, 4), pos, tri)
    with pytest.raises(RuntimeError, match="no CPU path"):
        md.visible_vertices(torch.zeros(8, 8, 4), tri, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        md.GBufferRenderer().render([torch.eye(4)], torch.zeros(3, 3), tri, None, (8, 8), ["mask"])
    # the camera of the reference's to_gl_camera: K, R, t -> projection @ diag(1, 1, -1, 1) @ [R | t]
    K = torch.tensor([[500.0, 0, 250.0], [0, 400.0, 260.0], [0, 0, 1]])
    P = md.GBufferRenderer.to_gl_camera(K, torch.eye(3), torch.tensor([0.1, 0.2, 3.0]), (512, 512), n=1.0, f=3.0)
    want = np.array([[1000 / 512, 0, 1 - 500 / 512, 0], [0, 800 / 512, 1 - 520 / 512, 0], [0, 0, -2.0, -3.0], [0, 0, -1, 0]])
    rt = np.eye(4)
    rt[:3, 3] = [0.1, 0.2, 3.0]
    assert np.allclose(P.numpy(), want @ np.diag([1.0, 1.0, -1.0, 1.0]) @ rt, rtol=1e-6, atol=1e-6)
