"""GPU checks of the deformer's geometry terms (garmentdreamer_amd/mesh_geometry.py, the entries of
include/gd_mesh_geometry.h in csrc/raster_geometry.hip) and of one deformer iteration (garmentdreamer_amd/deformer.py)
against the float64 statement of tests/mesh_geometry_reference.py.

Tolerance: the normalised error max|g - g64| / max|g64|.  The test evaluates the SAME reference in float32 on the CPU on the
same input, measures its normalised error against float64, and allows the GPU four times that: the kernels sum in another
order (gather in CSR order, a fixed tree) and are built without contraction.  For a scalar loss the float32 reference's
error is the largest over three summation orders (mesh_geometry_reference.scalar_sums).  Every figure is printed.

Shapes: a single triangle; a two-triangle quad; the 576-triangle tube(24, 12) with seeded N(0, 0.01) noise; a 100-triangle
fan around one vertex (a valence above a wave's 64 lanes); tube(96, 64), V = 6 240 (no multiple of 256) and F = 12 288:
25 and 48 workgroups, so the two-level reductions and their tails are exercised."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import mesh_geometry_reference as gref
from tests import mesh_scenes as scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ["single", "quad", "tube24", "fan100", "tube96"]
WEIGHTS = {"normal_consistency": 0.1, "laplacian": 800.0}      # the deformer's; sum w vn enters with weight 1


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mesh(name):
    if name == "single":
        return gref.SINGLE[0].astype(np.float32), gref.SINGLE[1]
    if name == "quad":
        return gref.QUAD[0].astype(np.float32), gref.QUAD[1]
    if name == "tube24":
        v, tri = gref.tube(24, 12)
        return gref.noisy(v, 0.01, seed=11), tri
    if name == "fan100":
        v, tri = gref.fan(100)
        return gref.noisy(v, 0.002, seed=12), tri
    v, tri = gref.tube(96, 64)
    assert v.shape[0] == 6240 and tri.shape[0] == 12288
    return gref.noisy(v, 0.002, seed=13), tri


def _reference(v32, tri, w_vn, dtype):
    """Forward values and the four gradients of the reference in ``dtype``; the losses as lists (scalar_sums)."""
    out = {}
    x = torch.from_numpy(v32).to(dtype)
    w = torch.from_numpy(w_vn).to(dtype)
    fn, vn = gref.normals(x, tri)
    out["fn"], out["vn"] = fn.numpy(), vn.numpy()
    nc_terms = gref.consistency_terms(fn, tri)
    out["laplacian"] = [float(s) / x.shape[0] for s in gref.scalar_sums(gref.laplacian_terms(x, tri))]
    out["normal_consistency"] = [float(s) / max(nc_terms.shape[0], 1) for s in gref.scalar_sums(nc_terms)]

    def grad(fn_):
        leaf = x.clone().requires_grad_(True)
        fn_(leaf).backward()
        return leaf.grad.numpy()

    def nc(a):
        return gref.consistency_loss(gref.normals(a, tri)[0], tri)

    out["d sum w vn"] = grad(lambda a: (gref.normals(a, tri)[1] * w).sum())
    out["d laplacian"] = grad(lambda a: gref.laplacian_loss(a, tri))
    out["d normal_consistency"] = grad(nc) if nc_terms.shape[0] else np.zeros(v32.shape)
    out["d weighted sum"] = grad(lambda a: (gref.normals(a, tri)[1] * w).sum() + WEIGHTS["normal_consistency"] * nc(a)
                                 + WEIGHTS["laplacian"] * gref.laplacian_loss(a, tri))
    return out


@functools.lru_cache(maxsize=None)
def _case(name):
    """Everything the CPU reference says about a shape; computed once, shared and treated as read-only."""
    v32, tri = _mesh(name)
    w_vn = np.random.RandomState(21).uniform(-1, 1, size=v32.shape).astype(np.float32)
    return dict(v=v32, tri=tri, w_vn=w_vn, r64=_reference(v32, tri, w_vn, torch.float64),
                r32=_reference(v32, tri, w_vn, torch.float32))


@functools.lru_cache(maxsize=None)
def _gpu_case(name):
    from garmentdreamer_amd import mesh_geometry as mg
    c = _case(name)
    return _dev(c["v"]), mg.build_geometry(c["tri"], num_vertices=c["v"].shape[0], device=DEV), _dev(c["w_vn"])


def _check(what, got, r64, r32):
    """The 4x rule of the module docstring; ``r64`` / ``r32`` arrays, or lists of scalars (the first is torch's own sum)."""
    if isinstance(r64, list):
        want = r64[0]
        e_gpu = abs(float(got) - want) / abs(want)
        e_f32 = max(abs(r - want) / abs(want) for r in r32)
    else:
        assert np.isfinite(got).all() and np.abs(r64).max() > 0
        e_gpu, e_f32 = gref.normalised_error(got, r64), gref.normalised_error(r32, r64)
    print(f"{what}: normalised error GPU {e_gpu:.3e}, float32 reference {e_f32:.3e}, allowed {4 * e_f32:.3e}")
    assert e_gpu <= 4 * e_f32, (what, e_gpu, e_f32)


@pytest.mark.parametrize("name", SHAPES)
def test_forward_against_the_float64_statement(name):
    from garmentdreamer_amd import mesh_geometry as mg
    c = _case(name)
    v, geo, _ = _gpu_case(name)
    fn, vn = mg.normals(v, geo)
    assert tuple(fn.shape) == (c["tri"].shape[0], 3) and tuple(vn.shape) == tuple(v.shape)
    _check(f"{name} fn", fn.cpu().numpy(), c["r64"]["fn"], c["r32"]["fn"])
    _check(f"{name} vn", vn.cpu().numpy(), c["r64"]["vn"], c["r32"]["vn"])
    lap = mg.laplacian_loss(v, geo)
    assert lap.dim() == 0 and lap.dtype == torch.float32
    _check(f"{name} laplacian loss", lap.item(), c["r64"]["laplacian"], c["r32"]["laplacian"])
    nc = mg.normal_consistency_loss(fn, geo)
    assert nc.dim() == 0
    if geo.num_pairs == 0:
        assert name == "single" and nc.item() == 0.0                   # no pair: exactly 0, not the reference's NaN
    else:
        _check(f"{name} normal consistency loss", nc.item(), c["r64"]["normal_consistency"],
               c["r32"]["normal_consistency"])
    mesh = mg.DeformMesh(v, _dev(c["tri"]), geo)                        # the Mesh-shaped surface gives the same bits
    assert torch.equal(mesh.face_normals, fn) and torch.equal(mesh.vertex_normals, vn)
    assert torch.equal(mg.laplacian_loss(mesh), lap) and torch.equal(mg.normal_consistency_loss(mesh), nc)
    assert mesh.indices.dtype == torch.int64 and torch.equal(mesh.edges, geo.edges)
    assert torch.equal(mesh.connected_faces, geo.connected_faces)


def _gpu_gradients(name):
    from garmentdreamer_amd import mesh_geometry as mg
    v, geo, w = _gpu_case(name)

    def grad(fn_):
        leaf = v.clone().requires_grad_(True)
        fn_(leaf).backward()
        return leaf.grad

    def nc(a):
        return mg.normal_consistency_loss(mg.normals(a, geo)[0], geo)

    def weighted(a):
        fn, vn = mg.normals(a, geo)
        return (vn * w).sum() + WEIGHTS["normal_consistency"] * mg.normal_consistency_loss(fn, geo) \
            + WEIGHTS["laplacian"] * mg.laplacian_loss(a, geo)

    return {"d sum w vn": grad(lambda a: (mg.normals(a, geo)[1] * w).sum()),
            "d laplacian": grad(lambda a: mg.laplacian_loss(a, geo)),
            "d normal_consistency": grad(nc),
            "d weighted sum": grad(weighted)}


@pytest.mark.parametrize("name", SHAPES)
def test_gradients_against_the_float64_statement(name):
    c = _case(name)
    got = _gpu_gradients(name)
    for key, g in got.items():
        assert tuple(g.shape) == c["v"].shape and g.dtype == torch.float32
        if key == "d normal_consistency" and name == "single":
            assert not g.any()                                           # no pair: exactly 0
            continue
        _check(f"{name} {key}", g.cpu().numpy(), c["r64"][key], c["r32"][key])


@pytest.mark.parametrize("name", ["tube24", "fan100", "tube96"])
def test_reruns_are_bit_identical(name):
    from garmentdreamer_amd import mesh_geometry as mg
    v, geo, _ = _gpu_case(name)
    first, second = _gpu_gradients(name), _gpu_gradients(name)
    for key in first:
        assert first[key].abs().max() > 0 and torch.equal(first[key].view(torch.int32), second[key].view(torch.int32)), key
    outs = []
    for _ in range(2):
        fn, vn = mg.normals(v, geo)
        outs.append((fn, vn, mg.laplacian_loss(v, geo), mg.normal_consistency_loss(fn, geo)))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_null_gradients():
    """dvn only, dfn only, both: a loss on one output reaches the kernel with a null pointer for the other."""
    from garmentdreamer_amd import mesh_geometry as mg
    c = _case("tube24")
    v, geo, w = _gpu_case("tube24")
    u_np = np.random.RandomState(22).uniform(-1, 1, size=(c["tri"].shape[0], 3)).astype(np.float32)
    u = _dev(u_np)
    cases = {"dvn only": lambda fn, vn, wv, wf: (vn * wv).sum(), "dfn only": lambda fn, vn, wv, wf: (fn * wf).sum(),
             "both": lambda fn, vn, wv, wf: (vn * wv).sum() + (fn * wf).sum()}
    for what, loss in cases.items():
        leaf = v.clone().requires_grad_(True)
        loss(*mg.normals(leaf, geo), w, u).backward()
        refs = []
        for dtype in (torch.float64, torch.float32):
            x = torch.from_numpy(c["v"]).to(dtype).requires_grad_(True)
            loss(*gref.normals(x, c["tri"]), torch.from_numpy(c["w_vn"]).to(dtype), torch.from_numpy(u_np).to(dtype)).backward()
            refs.append(x.grad.numpy())
        _check(what, leaf.grad.cpu().numpy(), refs[0], refs[1])


def _raw(v, geo, dvn, dfn):
    """Every entry called directly with its outputs pre-filled with NaN."""
    from garmentdreamer_amd import _native
    L = _native.lib()
    s = torch.cuda.current_stream(DEV).cuda_stream
    V, F, N = v.shape[0], geo.tri.shape[0], geo.nbr_idx.shape[0]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)      # noqa: E731
    o = dict(fn=nan(F, 3), vn=nan(V, 3), len=nan(V), dverts=nan(V, 3), delta=nan(V, 3), lap=nan(1), dlap=nan(V, 3),
             nc=nan(1), dnc=nan(F, 3))
    topo = geo.topology
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())                          # noqa: E731
    scratch = nan(max(L.gd_mesh_normals_backward_scratch_bytes(F), L.gd_mesh_loss_scratch_bytes(max(V, F))) // 4 + 1)
    one = torch.ones(1, dtype=torch.float32, device=DEV)
    assert L.gd_mesh_normals_forward(s, V, F, p(v), p(geo.tri), p(topo.corner_ptr), p(topo.corner_idx), p(o["fn"]),
                                     p(o["vn"]), p(o["len"])) == 0
    assert L.gd_mesh_normals_backward(s, V, F, p(v), p(geo.tri), p(topo.corner_ptr), p(topo.corner_idx), p(o["vn"]),
                                      p(o["len"]), p(dvn), p(dfn), p(o["dverts"]), p(scratch)) == 0
    assert L.gd_mesh_laplacian_forward(s, V, N, p(v), p(geo.nbr_ptr), p(geo.nbr_idx), p(o["delta"]), p(o["lap"]),
                                       p(scratch)) == 0
    assert L.gd_mesh_laplacian_backward(s, V, N, p(geo.nbr_ptr), p(geo.nbr_idx), p(o["delta"]), p(one), p(o["dlap"])) == 0
    assert L.gd_mesh_normal_consistency_forward(s, F, geo.num_pairs, p(o["fn"]), p(geo.face_nbr), p(o["nc"]),
                                                p(scratch)) == 0
    assert L.gd_mesh_normal_consistency_backward(s, F, geo.num_pairs, p(o["fn"]), p(geo.face_nbr), p(one),
                                                 p(o["dnc"])) == 0
    return o


def test_every_output_element_is_written_and_unused_vertices_get_zero():
    from garmentdreamer_amd import mesh_geometry as mg
    v0, tri = gref.tube(6, 3)
    V = v0.shape[0] + 2                                                  # two vertices no face uses: isolated, no corner
    extra = np.array([[0.7, -0.2, 0.4], [-0.3, 0.6, 0.1]])
    v = _dev(np.concatenate((gref.noisy(v0, 0.01, seed=31), extra.astype(np.float32))))
    geo = mg.build_geometry(tri, num_vertices=V, device=DEV)
    rng = np.random.RandomState(32)
    dvn, dfn = _dev(rng.uniform(-1, 1, (V, 3)).astype(np.float32)), _dev(rng.uniform(-1, 1, (len(tri), 3)).astype(np.float32))
    o = _raw(v, geo, dvn, dfn)
    for key, t in o.items():
        assert torch.isfinite(t).all(), key
    assert not o["vn"][-2:].any() and not o["len"][-2:].any()           # no corner: vn = 0
    assert torch.equal(o["delta"][-2:], -v[-2:])                         # isolated: delta = -v
    assert not o["dverts"][-2:].any()                                    # exactly 0
    assert torch.equal(o["dlap"][-2:], (2.0 / V) * v[-2:])               # dv = (2 / V) (0 - delta)
    assert o["dverts"][:-2].abs().min() > 0 and o["dnc"].abs().max() > 0
    # a mesh without a face and one without a pair
    none = mg.build_geometry(np.zeros((0, 3), np.int64), num_vertices=V, device=DEV)
    o = _raw(v, none, dvn, torch.zeros(1, 3, device=DEV))
    assert not o["vn"].any() and not o["dverts"].any() and o["nc"].item() == 0.0 and torch.equal(o["delta"], -v)
    single = mg.build_geometry(gref.SINGLE[1], device=DEV)
    o = _raw(_dev(gref.SINGLE[0].astype(np.float32)), single, None, None)
    assert o["nc"].item() == 0.0 and not o["dnc"].any() and not o["dverts"].any()


def test_a_zero_area_face_changes_nothing_and_every_gradient_stays_finite():
    from garmentdreamer_amd import mesh_geometry as mg
    v0, tri = gref.tube(6, 3)
    base = gref.noisy(v0, 0.01, seed=41)
    d = np.array([0.0078125, -0.015625, 0.00390625], np.float32)         # powers of two: a + d and a + 2 d are exact
    v_np = np.concatenate((base, (base[0] + d)[None], (base[0] + 2 * d)[None])).astype(np.float32)
    assert np.array_equal(v_np[-2] - v_np[0], d) and np.array_equal(v_np[-1] - v_np[0], 2 * d)
    V = v_np.shape[0]
    flat = np.concatenate((tri, np.array([[0, V - 2, V - 1]])))           # collinear corners, listed last
    v = _dev(v_np)
    with_face = mg.build_geometry(flat, num_vertices=V, device=DEV)
    without = mg.build_geometry(tri, num_vertices=V, device=DEV)
    leaf = v.clone().requires_grad_(True)
    fn, vn = mg.normals(leaf, with_face)
    _, vn_without = mg.normals(v, without)
    assert not fn[-1].any()                                              # exactly 0
    assert torch.equal(vn[:-2].detach().view(torch.int32), vn_without[:-2].view(torch.int32))
    assert not vn[-2:].any()                                             # vertices of the zero-area face only
    w = _dev(np.random.RandomState(42).uniform(-1, 1, (V, 3)).astype(np.float32))
    ((vn * w).sum() + mg.normal_consistency_loss(fn, with_face) + mg.laplacian_loss(leaf, with_face)).backward()
    assert torch.isfinite(leaf.grad).all() and leaf.grad.abs().max() > 0


# ---- one deformer iteration ------------------------------------------------------------------------------------------------

RES = (64, 64)


@functools.lru_cache(maxsize=None)
def _deformer_scene():
    from garmentdreamer_amd import mesh_deform as md
    v, tri, _ = scenes.tube()
    mvp = scenes.perspective(scenes.FOVY) @ np.linalg.inv(scenes.look_at_pose(scenes.CAMPOS))
    mvps = [_dev(mvp.astype(np.float32)), _dev((mvp @ np.diag([-1.0, 1, 1, 1])).astype(np.float32))]
    v_d, tri_d = _dev(v.astype(np.float32)), _dev(tri.astype(np.int32))
    moved = v_d + torch.tensor([0.05, 0.0, 0.0], device=DEV)
    with torch.no_grad():
        targets = [g["mask"] for g in md.GBufferRenderer().render(mvps, moved, tri_d, None, RES, ["mask"])]
    return v_d, tri_d, mvps, targets


def _deformer():
    from garmentdreamer_amd.deformer import Deformer
    v, tri, mvps, targets = _deformer_scene()
    return Deformer(v, tri, mvps, targets, RES)


def test_deformer_descends_and_is_reproducible():
    runs = []
    for _ in range(2):
        d = _deformer()
        losses = [d.step([0, 1]) for _ in range(30)]
        runs.append((d.offsets.detach().clone(), losses))
    offsets, losses = runs[0]
    first, last = losses[0]["mask"].item(), losses[-1]["mask"].item()
    print("mask loss at step 1", first, "after 30 steps", last)
    assert sorted(losses[0]) == ["laplacian", "mask", "normal_consistency", "total"]
    assert all(not t.requires_grad and t.is_cuda for t in losses[0].values())
    assert first > 0 and last < first
    assert torch.isfinite(offsets).all() and offsets.abs().max() > 0
    assert torch.equal(offsets.view(torch.int32), runs[1][0].view(torch.int32))


def test_deformer_only_visible_is_one_step_of_a_fresh_adam_on_the_visible_rows():
    d = _deformer()
    for _ in range(2):
        d.step([0, 1])
    before = d.offsets.detach().clone()
    d.step([0], only_visible=True)
    g = d.offsets.grad
    visible = d.renderer.vertex_visibility([d.mvps[0]], d.initial + before, d.geometry.tri, [RES])
    n = int(visible.sum())
    print("visible vertices", n, "of", visible.shape[0])
    assert 0 < n < visible.shape[0]
    after = d.offsets.detach()
    assert torch.equal(after[~visible].view(torch.int32), before[~visible].view(torch.int32))
    want = before - d.lr * g / (g.abs() + 1e-8)
    assert torch.equal(after[visible], want[visible]) and not torch.equal(after[visible], before[visible])


def test_deformer_step_does_not_synchronise():
    d = _deformer()
    for _ in range(2):
        d.step([0, 1])
        d.step([0, 1], only_visible=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = d.step([0, 1])
        out_visible = d.step([0, 1], only_visible=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(out["total"]).item() and torch.isfinite(out_visible["total"]).item()
