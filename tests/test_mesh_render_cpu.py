"""CPU-side checks of the mesh render path: the gd_mesh_* boundary (include/gd_mesh.h) is exported, bound and validates
its arguments without a GPU; the host topology of ``build_topology``; the camera matrices; and the numpy reference
(tests/mesh_reference.py) itself on cases that can be checked by hand."""
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_reference as ref
from tests import mesh_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mesh_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gd_mesh.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gd_mesh_[a-z0-9_]+)\s*\(", text)))
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert len(declared) == 8
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_mesh.h but not exported"
    assert sorted(_native.MESH_SIGNATURES) == declared
    # argument validation before any device work
    assert L.gd_mesh_rasterize(None, 3, 1, 0, 64, None, None, None, None) == -1
    assert b"positive" in L.gd_mesh_last_error()
    assert L.gd_mesh_rasterize(None, 3, 1 << 24, 8, 8, None, None, None, None) == -1 and b"2^24" in L.gd_mesh_last_error()
    assert L.gd_mesh_rasterize(None, 3, 1, 8, 8, None, None, None, None) == -1 and b"null" in L.gd_mesh_last_error()
    assert L.gd_mesh_interpolate_forward(None, 3, 1, 9, 8, 8, None, None, None, None) == -1
    assert b"[1, 8]" in L.gd_mesh_last_error()
    assert L.gd_mesh_interpolate_backward(None, 3, 1, 0, 8, 8, *([None] * 8)) == -1
    assert L.gd_mesh_antialias_weights(None, 3, 1, 8, 8, *([None] * 5)) == -1
    assert L.gd_mesh_antialias_apply(None, 3, 8, 8, None, None, None, 0) == -1
    # scratch: the u64 visibility buffer + the large-triangle list; the [F][3][C] slab
    assert L.gd_mesh_rasterize_scratch_bytes(1000, 512, 512) >= 512 * 512 * 8 + 1000 * 4
    assert L.gd_mesh_interpolate_backward_scratch_bytes(1000, 3) >= 1000 * 9 * 4


def test_ops_reject_cpu_tensors_and_bad_arguments():
    from garmentdreamer_amd import mesh_render as mr
    pos, tri = torch.zeros(3, 4), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mr.rasterize(pos, tri, (8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mr.interpolate(torch.zeros(3, 3), torch.zeros(8, 8, 4), tri)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mr.antialias(torch.zeros(8, 8, 3), torch.zeros(8, 8, 4), pos, tri)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mr.MeshRenderer(torch.zeros(3, 3), tri, torch.zeros(3, 3), lambda x: x)


def _check_csr(topo, tri, V):
    ptr, idx = topo.corner_ptr.numpy(), topo.corner_idx.numpy()
    assert ptr.dtype == np.int32 and idx.dtype == np.int32
    assert ptr.shape == (V + 1,) and ptr[0] == 0 and ptr[-1] == 3 * tri.shape[0] and np.all(np.diff(ptr) >= 0)
    assert np.array_equal(np.sort(idx), np.arange(3 * tri.shape[0]))             # each corner exactly once
    flat = tri.ravel()
    for v in range(V):
        mine = idx[ptr[v]:ptr[v + 1]]
        assert np.all(flat[mine] == v) and np.all(np.diff(mine) > 0)               # its own corners, ascending


def test_build_topology_quad():
    from garmentdreamer_amd.mesh_render import build_topology
    tri = np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)
    topo = build_topology(tri)
    assert topo.opp.dtype == torch.int32
    # the diagonal (0, 2) is edge 1 of triangle 0 (opposite vertex 1) and edge 2 of triangle 1 (opposite vertex 3)
    assert topo.opp.tolist() == [[-1, 3, -1], [-1, -1, 1]]
    _check_csr(topo, tri, 4)
    assert topo.corner_ptr.tolist() == [0, 2, 3, 5, 6] and topo.corner_idx.tolist() == [0, 3, 1, 2, 4, 5]
    # an isolated vertex has an empty list; an index past num_vertices is refused
    assert build_topology(tri, num_vertices=6).corner_ptr.tolist() == [0, 2, 3, 5, 6, 6, 6]
    with pytest.raises(ValueError, match="out of range"):
        build_topology(tri, num_vertices=3)
    # three triangles on one edge: nobody has a unique neighbour across it
    fan = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int32)
    assert build_topology(fan).opp.tolist() == [[-1, -1, -1]] * 3


def test_build_topology_tube():
    from garmentdreamer_amd.mesh_render import build_topology
    v, tri, _ = scenes.tube()
    topo = build_topology(torch.from_numpy(tri), num_vertices=v.shape[0])
    opp = topo.opp.numpy()
    assert np.array_equal(opp, ref.build_opposite(tri))                            # against a dictionary walk
    # an open tube of 24 x 12 quads: 2 x 24 rim edges are boundaries, everything else has a neighbour
    assert (opp < 0).sum() == 48
    for t, i in ((0, 0), (100, 1), (575, 2)):
        d = opp[t, i]
        edge = {int(tri[t, (i + 1) % 3]), int(tri[t, (i + 2) % 3])}
        if d >= 0:
            other = [u for u in range(tri.shape[0]) if u != t and edge <= set(tri[u].tolist())]
            assert len(other) == 1 and d in tri[other[0]] and d not in edge
    _check_csr(topo, tri, v.shape[0])


def test_projection_and_perspective_values():
    from garmentdreamer_amd.mesh_render import perspective, projection
    p = perspective(np.pi / 2)                                                     # tan(fovy / 2) = 1
    assert p.dtype == np.float32 and p.shape == (4, 4)
    want = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -100.01 / 99.99, -2.0 / 99.99], [0, 0, -1, 0]])
    assert np.allclose(p, want, rtol=1e-6, atol=0)
    assert np.array_equal(perspective(0.75), scenes.perspective(0.75))
    q = projection(fx=500.0, fy=400.0, cx=250.0, cy=260.0, width=512, height=512)  # n = 0.01, f = 1000
    want = np.array([[1000 / 512, 0, 1 - 500 / 512, 0], [0, 800 / 512, 1 - 520 / 512, 0],
                     [0, 0, -1000.01 / 999.99, -20.0 / 999.99], [0, 0, -1, 0]])
    assert q.dtype == np.float32 and np.allclose(q, want, rtol=1e-6, atol=1e-9)
    assert np.allclose(projection(1, 1, 0, 0, 2, 2, n=1.0, f=3.0)[2], [0, 0, -2.0, -3.0])


def test_reference_right_triangle_coverage():
    """Corners on pixel corners (0,0), (4,0), (0,4) of an 8 x 8 frame: the centres with c + r <= 2 are inside (6); the
    four with c + r = 3 lie ON the hypotenuse, whose normalised edge vector (-1024, +1024) has dY > 0, so they count."""
    pos = np.array([[-1, -1, 0, 1], [0, -1, 0, 1], [-1, 0, 0, 1]], dtype=np.float32)
    rast = ref.rasterize(pos, np.array([[0, 1, 2]]), 8, 8)
    cov = rast[..., 3] > 0
    rr, cc = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    assert cov.sum() == 10 and np.array_equal(cov, rr + cc <= 3)
    # the other winding covers the same pixels; barycentrics at pixel (0, 0): centre (0.5, 0.5) of a 4-pixel leg
    flipped = ref.rasterize(pos, np.array([[0, 2, 1]]), 8, 8)
    assert np.array_equal(flipped[..., 3] > 0, cov)
    assert rast[0, 0].tolist() == [0.75, 0.125, 0.0, 1.0]
    assert np.all(rast[~cov] == 0)


@pytest.mark.parametrize("split", [[[0, 1, 2], [0, 2, 3]], [[0, 1, 3], [1, 2, 3]], [[2, 1, 0], [0, 2, 3]]])
def test_reference_quad_split_on_a_diagonal_covers_each_pixel_once(split):
    """The diagonal passes through pixel centres: every one of them belongs to exactly one of the two triangles."""
    pos = np.array([[-1, -1, 0.5, 1], [1, -1, 0.5, 1], [1, 1, 0.5, 1], [-1, 1, 0.5, 1]], dtype=np.float32)
    tri = np.array(split)
    n = np.zeros((8, 8), dtype=int)
    for t in range(2):
        n += ref.rasterize(pos, tri[t:t + 1], 8, 8)[..., 3] > 0
    assert np.array_equal(n, np.ones((8, 8), dtype=int))
    both = ref.rasterize(pos, tri, 8, 8)
    assert (both[..., 3] == 1).sum() + (both[..., 3] == 2).sum() == 64 and (both[..., 3] == 1).sum() in (28, 36)


def test_reference_drops_and_depth_rules():
    pos, tri, names = scenes.edge_case_scene()
    rast = ref.rasterize(pos, tri, 48, 64)
    ids = rast[..., 3].astype(int) - 1
    for gone in ("dup_1", "zero_area", "behind", "w_zero", "wholly_out"):
        assert not (ids == names[gone]).any(), gone
    for seen in ("large_a", "large_b", "dup_0", "partly_out", "z_range", "w_varies"):
        assert (ids == names[seen]).any(), seen
    assert (ids[ids >= 0] < 576).any()
    assert np.all(rast[..., 2] >= -1) and np.all(rast[..., 2] <= 1)
    # the windowed evaluation is the same function
    assert np.array_equal(ref.rasterize(pos, tri, 48, 64, window=8).view(np.uint32), rast.view(np.uint32))


def test_reference_antialias_adjoint_is_the_transpose_of_apply():
    pos, tri, _ = scenes.edge_case_scene()
    rast = ref.rasterize(pos, tri, 48, 64)
    wts = ref.antialias_weights(rast, pos, tri, ref.build_opposite(tri))
    assert (wts >= 0).all() and (wts <= 0.5).all() and (wts != 0).sum() >= 50
    rng = np.random.RandomState(0)
    x, y = rng.rand(48, 64, 3).astype(np.float32), rng.rand(48, 64, 3).astype(np.float32)
    lhs = (ref.antialias_apply(x, wts).astype(np.float64) * y).sum()
    rhs = (x.astype(np.float64) * ref.antialias_adjoint(y, wts)).sum()
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs)
