"""CPU-side checks of the deformer's geometry terms: the entries of include/gd_mesh_geometry.h are exported, bound and
validate their arguments without a GPU; ``build_geometry`` agrees with the numpy statement of the connectivity; the
REFERENCE (tests/mesh_geometry_reference.py) is pinned itself, its two forms against each other and its float64 autograd
gradients against central differences; the fresh-Adam identity that ``Deformer.step(only_visible=True)`` rests on."""
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_geometry_reference as gref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_geometry_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gd_mesh_geometry.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gd_mesh_[a-z0-9_]+)\s*\(", text)))
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert len(declared) == 8
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_mesh_geometry.h but not exported"
    assert sorted(_native.MESH_GEOMETRY_SIGNATURES) == declared
    # the three headers of the mesh path declare disjoint sets
    assert not set(declared) & (set(_native.MESH_SIGNATURES) | set(_native.MESH_DEFORM_SIGNATURES))


def test_scratch_queries():
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert L.gd_mesh_normals_backward_scratch_bytes(1000) >= 1000 * 12 * 4      # the [F][3][4] slab
    assert L.gd_mesh_normals_backward_scratch_bytes(0) == 0
    assert L.gd_mesh_normals_backward_scratch_bytes(-1) == 0
    assert L.gd_mesh_loss_scratch_bytes(6240) >= 25 * 4                           # one partial per 256 elements
    assert L.gd_mesh_loss_scratch_bytes(1) >= 4
    assert L.gd_mesh_loss_scratch_bytes(-5) == 0


def test_entries_validate_their_arguments():
    """-1 and a message before any device work: null pointers, V <= 0, F < 0 (no GPU is touched: the stream is never used)."""
    from garmentdreamer_amd import _native
    L = _native.lib()
    err = L.gd_mesh_last_error
    x = 0x1000                                     # a non-null pointer that is never followed
    for V, F in ((0, 1), (-3, 1), (3, -1)):
        assert L.gd_mesh_normals_forward(None, V, F, *([x] * 7)) == -1 and b"normals" in err()
        assert L.gd_mesh_normals_backward(None, V, F, *([x] * 10)) == -1 and b"normals backward" in err()
    assert L.gd_mesh_normals_forward(None, 3, 1, *([None] * 7)) == -1 and b"null" in err()
    for hole in range(7):                          # each pointer on its own
        args = [x] * 7
        args[hole] = None
        assert L.gd_mesh_normals_forward(None, 3, 1, *args) == -1 and b"null" in err(), hole
    assert L.gd_mesh_normals_backward(None, 3, 1, *([None] * 10)) == -1 and b"null" in err()
    for hole in (0, 1, 2, 3, 8, 9):                # verts tri ptr idx . . . . dverts scratch; dvn / dfn may be null
        args = [x] * 10
        args[hole] = None
        assert L.gd_mesh_normals_backward(None, 3, 1, *args) == -1 and b"null" in err(), hole
    args = [x] * 10
    args[4] = None                                 # dvn given without the vn it needs
    assert L.gd_mesh_normals_backward(None, 3, 1, *args) == -1 and b"null" in err()
    for V in (0, -1):
        assert L.gd_mesh_laplacian_forward(None, V, 6, *([x] * 6)) == -1 and b"laplacian" in err()
        assert L.gd_mesh_laplacian_backward(None, V, 6, *([x] * 5)) == -1 and b"laplacian backward" in err()
    assert L.gd_mesh_laplacian_forward(None, 3, -1, *([x] * 6)) == -1
    assert L.gd_mesh_laplacian_forward(None, 3, 6, *([None] * 6)) == -1 and b"null" in err()
    assert L.gd_mesh_laplacian_backward(None, 3, 6, *([None] * 5)) == -1 and b"null" in err()
    for hole in range(6):
        args = [x] * 6
        args[hole] = None
        assert L.gd_mesh_laplacian_forward(None, 3, 6, *args) == -1 and b"null" in err(), hole
    for hole in range(5):
        args = [x] * 5
        args[hole] = None
        assert L.gd_mesh_laplacian_backward(None, 3, 6, *args) == -1 and b"null" in err(), hole
    assert L.gd_mesh_normal_consistency_forward(None, -1, 0, *([x] * 4)) == -1 and b"consistency" in err()
    assert L.gd_mesh_normal_consistency_forward(None, 2, -1, *([x] * 4)) == -1
    assert L.gd_mesh_normal_consistency_backward(None, -1, 0, *([x] * 4)) == -1 and b"consistency backward" in err()
    assert L.gd_mesh_normal_consistency_backward(None, 2, -1, *([x] * 4)) == -1
    assert L.gd_mesh_normal_consistency_forward(None, 2, 1, *([None] * 4)) == -1 and b"null" in err()
    assert L.gd_mesh_normal_consistency_backward(None, 2, 1, *([None] * 4)) == -1 and b"null" in err()
    for hole in range(4):
        args = [x] * 4
        args[hole] = None
        assert L.gd_mesh_normal_consistency_forward(None, 2, 1, *args) == -1 and b"null" in err(), hole
        assert L.gd_mesh_normal_consistency_backward(None, 2, 1, *args) == -1 and b"null" in err(), hole


UNUSED = np.array([[0, 1, 2], [0, 2, 4]], dtype=np.int64)                 # vertex 3 (and 5, with num_vertices = 6) unused
DUPLICATE = np.array([[0, 1, 2], [2, 1, 0]], dtype=np.int64)             # one face twice (opposite winding)


def _check_geometry(tri, V, E, P):
    from garmentdreamer_amd import mesh_geometry as mg
    from garmentdreamer_amd import mesh_render as mr
    geo = mg.build_geometry(torch.from_numpy(tri), num_vertices=V)
    F = tri.shape[0]
    assert geo.num_vertices == V and geo.num_pairs == P
    assert geo.tri.dtype == torch.int32 and np.array_equal(geo.tri.numpy(), tri)
    topo = mr.build_topology(tri, num_vertices=V)
    for got, want in zip(geo.topology, topo):
        assert torch.equal(got, want)
    assert geo.edges.dtype == torch.int64 and tuple(geo.edges.shape) == (E, 2)
    np.testing.assert_array_equal(geo.edges.numpy(), gref.edges_numpy(tri))
    assert geo.connected_faces.dtype == torch.int64 and tuple(geo.connected_faces.shape) == (P, 2)
    np.testing.assert_array_equal(geo.connected_faces.numpy(), gref.connected_faces_numpy(tri))
    assert geo.face_nbr.dtype == torch.int32 and tuple(geo.face_nbr.shape) == (F, 3)
    np.testing.assert_array_equal(geo.face_nbr.numpy(), gref.face_neighbours_numpy(tri))
    assert int((geo.face_nbr.numpy() > np.arange(F)[:, None]).sum()) == P    # the kernels' count of pairs: from the side f < g
    nbr = gref.neighbours_numpy(tri, V)
    ptr, idx = geo.nbr_ptr.numpy(), geo.nbr_idx.numpy()
    assert ptr.dtype == np.int32 and idx.dtype == np.int32 and ptr.shape == (V + 1,) and ptr[0] == 0
    assert [idx[ptr[i]:ptr[i + 1]].tolist() for i in range(V)] == nbr
    return geo


def test_build_geometry_quad():
    geo = _check_geometry(gref.QUAD[1], 4, 5, 1)
    assert geo.connected_faces.tolist() == [[0, 1]]                       # the reference's own expectation (geometry.py)
    assert geo.edges.tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [2, 3]]


def test_build_geometry_tube():
    v, tri = gref.tube(24, 12)
    assert v.shape[0] == 312 and tri.shape[0] == 576
    geo = _check_geometry(tri, 312, 888, 840)
    deg = np.diff(geo.nbr_ptr.numpy())
    assert deg.min() == 4 and deg.max() == 6 and deg.sum() == 2 * 888     # the open ends; the interior of a regular tube


def test_build_geometry_unused_vertex():
    geo = _check_geometry(UNUSED, 6, 5, 1)
    deg = np.diff(geo.nbr_ptr.numpy())
    assert deg[3] == 0 and deg[5] == 0
    assert np.diff(geo.topology.corner_ptr.numpy())[[3, 5]].tolist() == [0, 0]


def test_build_geometry_duplicated_face_gives_three_pairs():
    geo = _check_geometry(DUPLICATE, 3, 3, 3)
    assert geo.connected_faces.tolist() == [[0, 1]] * 3
    assert (geo.face_nbr.numpy() == np.array([[1, 1, 1], [0, 0, 0]])).all()


def test_build_geometry_refuses_a_three_triangle_fan_around_one_edge():
    from garmentdreamer_amd import mesh_geometry as mg
    tri = np.array([[0, 1, 2], [0, 1, 3], [0, 1, 4]])
    with pytest.raises(ValueError, match="more than two"):
        mg.build_geometry(tri)
    with pytest.raises(ValueError, match="out of range"):
        mg.build_geometry(np.array([[0, 1, 7]]), num_vertices=3)


# ---- the reference, pinned ------------------------------------------------------------------------------------------------

def _small_meshes():
    v, tri = gref.tube(6, 3)
    return [("single", *gref.SINGLE), ("quad", *gref.QUAD), ("tube", v, tri), ("fan", *gref.fan(9)),
            ("unused", np.random.RandomState(4).normal(size=(6, 3)), UNUSED)]


def test_reference_scatter_forms_agree_with_loops_and_the_dense_matrix():
    """float64; both forms evaluate the same expression per element and differ in summation order only: a few ulp."""
    for name, v, tri in _small_meshes():
        v = torch.from_numpy(gref.noisy(v, seed=1)).double()
        fn, vn = gref.normals(v, tri)
        fn_l, vn_l = gref.normals_looped(v, tri)
        assert float((fn - fn_l).abs().max()) <= 1e-14 and float((vn - vn_l).abs().max()) <= 1e-14, name
        assert abs(float(gref.laplacian_loss(v, tri)) - float(gref.laplacian_loss_dense(v, tri))) <= 1e-14, name
        assert abs(float(gref.consistency_loss(fn, tri)) - float(gref.consistency_loss_looped(fn, tri))) <= 1e-14, name
    # the statements that cannot be read off the formulas
    v = torch.from_numpy(gref.noisy(np.random.RandomState(4).normal(size=(6, 3)), seed=1)).double()
    fn, vn = gref.normals(v, UNUSED)
    assert not vn[3].any() and not vn[5].any()                            # no corner: vn = 0
    d = gref.laplacian_dense(UNUSED, 6, torch.float64) @ v
    assert torch.equal(d[3], -v[3]) and torch.equal(d[5], -v[5])          # isolated: delta = -v
    assert float(gref.consistency_loss(gref.normals(torch.from_numpy(gref.SINGLE[0]), gref.SINGLE[1])[0],
                                       gref.SINGLE[1])) == 0.0            # P = 0 gives 0
    # a duplicated face with the opposite winding: cos = -1 on each of its three pairs
    fn = gref.normals(torch.from_numpy(gref.SINGLE[0]), DUPLICATE)[0]
    assert abs(float(gref.consistency_loss(fn, DUPLICATE)) - 4.0) <= 1e-14


def _central_differences(fn, x, h):
    g = np.zeros(x.shape)
    for i in range(x.shape[0]):
        for j in range(x.shape[1]):
            lo, hi = x.copy(), x.copy()
            lo[i, j] -= h
            hi[i, j] += h
            g[i, j] = (fn(hi) - fn(lo)) / (2 * h)
    return g


def test_reference_autograd_gradients_agree_with_central_differences():
    v0, tri = gref.tube(6, 3)
    v0 = gref.noisy(v0, seed=2).astype(np.float64)
    rng = np.random.RandomState(3)
    w_vn, w_fn = rng.uniform(-1, 1, size=v0.shape), rng.uniform(-1, 1, size=(tri.shape[0], 3))
    t = torch.from_numpy

    def weighted_vn(x):
        return (gref.normals(x, tri)[1] * t(w_vn)).sum()

    def weighted_fn(x):
        return (gref.normals(x, tri)[0] * t(w_fn)).sum()

    def consistency(x):
        return gref.consistency_loss(gref.normals(x, tri)[0], tri)

    def laplacian(x):
        return gref.laplacian_loss(x, tri)

    def deformer_sum(x):
        return 0.1 * consistency(x) + 800 * laplacian(x) + weighted_vn(x)

    # 1e-6 steps of quantities of order 1 in float64: truncation ~1e-12, rounding ~1e-16 * |L| / 1e-6 ~ 1e-8 relative
    for name, fn in (("sum w vn", weighted_vn), ("sum w fn", weighted_fn), ("normal consistency", consistency),
                     ("laplacian", laplacian), ("weighted sum", deformer_sum)):
        x = t(v0).clone().requires_grad_(True)
        fn(x).backward()
        grad = x.grad.numpy()
        fd = _central_differences(lambda a: float(fn(t(a))), v0, 1e-6)
        err = np.abs(fd - grad).max() / np.abs(grad).max()
        print(name, "max |fd - autograd| / max |autograd|", err)
        assert np.abs(grad).max() > 0 and err <= 1e-6


def test_one_step_of_a_fresh_adam_is_lr_g_over_abs_g_plus_eps():
    """What Deformer.step(only_visible=True) applies.  float64: the identity holds to rounding (a dozen operations at
    2^-53 each, asserted at 1e-12 of the step); float32: the same at 2^-24 each, asserted at 2e-6 of the step.  The
    parameter starts at 0, so that the subtraction from it adds no rounding of its own to what is compared."""
    lr, eps = 1e-3, 1e-8
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2e-6)):
        torch.manual_seed(5)
        p0 = torch.zeros(200, 3, dtype=dtype)
        g = torch.randn(200, 3, dtype=dtype) * torch.logspace(-6, 2, 200, dtype=dtype)[:, None]
        p = p0.clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=lr)              # torch's default betas and eps, as the reference
        p.grad = g.clone()
        opt.step()
        want = p0 - lr * g / (g.abs() + eps)
        step = (p.detach() - p0).abs()
        assert float(step.max()) > 0.5 * lr
        assert float(((p.detach() - want).abs() / lr).max()) <= tol


def test_ops_reject_cpu_tensors():
    from garmentdreamer_amd import mesh_geometry as mg
    from garmentdreamer_amd.deformer import Deformer
    geo = mg.build_geometry(gref.QUAD[1])
    v = torch.from_numpy(gref.QUAD[0]).float().requires_grad_(True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mg.normals(v, geo)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mg.laplacian_loss(v, geo)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mg.normal_consistency_loss(torch.zeros(2, 3), geo)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mg.DeformMesh(v, torch.from_numpy(gref.QUAD[1]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        Deformer(v, torch.from_numpy(gref.QUAD[1]), [torch.eye(4)], [torch.zeros(8, 8, 1)], (8, 8))
    # mask_loss is plain torch: the mean over the views of the per-view MSE
    a, b = torch.rand(4, 4, 1), torch.rand(4, 4, 1)
    got = mg.mask_loss([a, b], [{"mask": b}, {"mask": a * 0}])
    assert abs(float(got) - float((((a - b) ** 2).mean() + (b ** 2).mean()) / 2)) <= 1e-7
