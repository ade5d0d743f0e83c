"""GPU checks of the mesh render path for moving geometry (garmentdreamer_amd/mesh_deform.py, the entries of
include/gd_mesh_deform.h in csrc/raster_mesh.hip): the forward is the fixed-geometry one bit for bit, and the gradients
to vertex positions agree with the float64 statement of tests/mesh_grad_reference.py.

Tolerance of the gradient comparisons: the normalised error max|g - g64| / max|g64|.  The test evaluates the SAME reference
in float32 on the CPU, measures its normalised error against float64, and allows the GPU four times that: the kernels sum in
another order (wave tree and CSR order against sequential) and are built without contraction.  Both figures are printed.

Scenes: tests/mesh_scenes.py's edge-case scene (the 576-triangle tube plus hand-placed triangles) at 64 x 48, the
three-triangle scene with edges above 16 pixels and a two-triangle quad of tests/mesh_grad_reference.py."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_grad_reference as gref
from tests import mesh_reference as ref
from tests import mesh_scenes as scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 48, 64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """Everything the CPU references say about a scene; shared and treated as read-only."""
    if name == "edge":
        pos, tri, names = scenes.edge_case_scene()
    else:
        (pos, tri), names = gref.big_triangle_scene(H, W), {}
    rast = ref.rasterize(pos, tri, H, W)
    opp = ref.build_opposite(tri)
    info = {}
    wts = ref.antialias_weights(rast, pos, tri, opp, info)
    pairs = gref.antialias_pairs(rast, pos, tri, opp)
    return dict(pos=pos, tri=tri, names=names, rast=rast, opp=opp, wts=wts, info=info, pairs=pairs)


@functools.lru_cache(maxsize=None)
def _gpu_scene(name):
    from garmentdreamer_amd import mesh_render as mr
    s = _scene(name)
    pos, tri = _dev(s["pos"]), _dev(s["tri"])
    return pos, tri, mr.build_topology(tri, num_vertices=pos.shape[0])


def _check_gradient(what, got, g64, g32):
    """The 4x rule of the module docstring."""
    e_gpu, e_f32 = gref.normalised_error(got, g64), gref.normalised_error(g32, g64)
    print(f"{what}: normalised error GPU {e_gpu:.3e}, float32 reference {e_f32:.3e}, allowed {4 * e_f32:.3e}")
    assert np.abs(g64).max() > 0 and np.isfinite(got).all()
    assert e_gpu <= 4 * e_f32, (what, e_gpu, e_f32)


def test_forward_is_the_fixed_geometry_forward_bit_for_bit():
    from garmentdreamer_amd import mesh_deform as md
    from garmentdreamer_amd import mesh_render as mr
    s = _scene("edge")
    pos, tri, topo = _gpu_scene("edge")
    want = mr.rasterize(pos, tri, (H, W))
    moving = pos.clone().requires_grad_(True)
    rast = md.rasterize(moving, tri, (H, W), topo)
    assert rast.requires_grad and torch.equal(rast.detach().view(torch.int32), want.view(torch.int32))
    np.testing.assert_array_equal(rast.detach().cpu().numpy().view(np.uint32), s["rast"].view(np.uint32))
    assert torch.equal(md.rasterize(moving, tri, (H, W)).detach().view(torch.int32), want.view(torch.int32))
    assert md.rasterize(moving[None], tri, (H, W)).shape == (1, H, W, 4)
    rng = np.random.RandomState(1)
    for C in (1, 3):
        x = _dev(rng.uniform(0, 1, size=(H, W, C)).astype(np.float32))
        aa_want = mr.antialias(x, want, pos, tri, topology=topo)
        aa = md.antialias(x, rast, moving, tri, topo)
        assert aa.requires_grad and torch.equal(aa.detach().view(torch.int32), aa_want.view(torch.int32))
        assert torch.equal(md.antialias(x, rast, moving, tri).detach().view(torch.int32), aa_want.view(torch.int32))
    a = _dev(rng.uniform(-1, 1, size=(pos.shape[0], 3)).astype(np.float32))
    assert torch.equal(md.interpolate(a, rast, tri, moving, topo).detach(), mr.interpolate(a, want, tri))


def _interpolate_rasterize_grad(name, attr, dout):
    from garmentdreamer_amd import mesh_deform as md
    pos, tri, topo = _gpu_scene(name)
    moving = pos.clone().requires_grad_(True)
    rast = md.rasterize(moving, tri, (H, W), topo)
    md.interpolate(_dev(attr), rast, tri, moving, topo).backward(_dev(dout))
    return moving.grad


@pytest.mark.parametrize("name,C", [("edge", 1), ("edge", 3), ("edge", 8), ("big", 3)])
def test_interpolate_gradient_to_rast_and_rasterize_backward(name, C):
    s = _scene(name)
    V = s["pos"].shape[0]
    rng = np.random.RandomState(20 + C)
    attr = rng.uniform(-1, 1, size=(V, C)).astype(np.float32)
    dout = rng.uniform(-1, 1, size=(H, W, C)).astype(np.float32)
    grad = _interpolate_rasterize_grad(name, attr, dout)
    assert tuple(grad.shape) == (V, 4) and grad.dtype == torch.float32
    got = grad.cpu().numpy()
    g64 = gref.grad_interpolate_rasterize(s["pos"], s["tri"], s["rast"], attr, dout, torch.float64)
    g32 = gref.grad_interpolate_rasterize(s["pos"], s["tri"], s["rast"], attr, dout, torch.float32)
    _check_gradient(f"interpolate o rasterize, {name}, C = {C}", got, g64, g32)
    assert not got[:, 2].any()                                           # z: exactly 0
    seen = np.zeros(V, bool)
    seen[s["tri"][np.unique(s["rast"][..., 3].astype(int))[1:] - 1].ravel()] = True
    assert not got[~seen].any() and (np.abs(got[seen]).sum(axis=1) > 0).mean() > 0.9
    if name == "edge":
        n = s["names"]
        for gone in ("zero_area", "behind", "w_zero", "wholly_out"):     # dropped triangles: exact-zero rows
            assert not got[s["tri"][n[gone]]].any(), gone
        assert np.all(got[s["tri"][n["w_varies"]], 3] != 0)               # the w derivative
        assert np.abs(g64[s["tri"][n["w_varies"]], 3]).min() > 0


def test_gradients_through_attr_and_through_rast_cancel():
    """L = sum_p c_p (P.x - fx P.w) with P = interpolate(attr = pos) is identically zero for the continuous (u, v)
    (sum_i a_i q_i = 0), so its gradient through attr and its gradient through rast cancel up to the snapping of the
    forward's (u, v).  The float64 reference shows that residual; the GPU may show twice as much."""
    from garmentdreamer_amd import mesh_deform as md
    s = _scene("big")
    pos, tri, topo = _gpu_scene("big")
    coeff = np.random.RandomState(3).uniform(-1, 1, size=(H, W)).astype(np.float32)
    fx = ((torch.arange(W, device=DEV, dtype=torch.float32) * 2 + 1) / W - 1)[None, :]

    def loss(P):
        return (_dev(coeff) * (P[..., 0] - fx * P[..., 3])).sum()

    a = pos.clone().requires_grad_(True)
    loss(md.interpolate(a, md.rasterize(pos, tri, (H, W)), tri, pos, topo)).backward()
    p = pos.clone().requires_grad_(True)
    loss(md.interpolate(pos, md.rasterize(p, tri, (H, W), topo), tri, p, topo)).backward()
    g_attr, g_rast = a.grad.double().cpu().numpy(), p.grad.double().cpu().numpy()
    r_attr, r_rast = gref.cancellation(s["pos"], s["tri"], s["rast"], coeff)
    res_gpu = np.abs(g_attr + g_rast).max() / np.abs(g_attr).max()
    res_ref = np.abs(r_attr + r_rast).max() / np.abs(r_attr).max()
    print(f"cancellation residual / max|gradient through attr|: GPU {res_gpu:.3e}, float64 reference {res_ref:.3e}")
    assert np.abs(g_attr).max() > 1 and np.abs(g_rast).max() > 1
    assert 0 < res_ref < 0.01 and res_gpu <= 2 * res_ref
    # both in one graph: the same leaf as attr and as pos
    both = pos.clone().requires_grad_(True)
    loss(md.interpolate(both, md.rasterize(both, tri, (H, W), topo), tri, both, topo)).backward()
    assert np.abs(both.grad.double().cpu().numpy()).max() <= 2 * res_ref * np.abs(g_attr).max() * (1 + 1e-3)


def _antialias_grad(name, color, dout):
    from garmentdreamer_amd import mesh_deform as md
    pos, tri, topo = _gpu_scene(name)
    moving = pos.clone().requires_grad_(True)
    rast = md.rasterize(pos, tri, (H, W))
    md.antialias(_dev(color), rast, moving, tri, topo).backward(_dev(dout))
    return moving.grad


@pytest.mark.parametrize("C", [1, 3])
def test_antialias_gradient_to_pos(C):
    s = _scene("edge")
    info = s["info"]
    assert min(info["to_outer"], info["to_inner"], info["horizontal"], info["vertical"], info["fold"],
               info["boundary"]) >= 1, info
    V = s["pos"].shape[0]
    rng = np.random.RandomState(30 + C)
    if C == 1:
        color = np.clip(s["rast"][..., 3:], 0, 1).astype(np.float32)     # the mask
    else:
        color = rng.uniform(0, 1, size=(H, W, C)).astype(np.float32)
    dout = rng.uniform(-1, 1, size=(H, W, C)).astype(np.float32)
    grad = _antialias_grad("edge", color, dout)
    assert tuple(grad.shape) == (V, 4)
    got = grad.cpu().numpy()
    g64 = gref.grad_antialias(s["pos"], s["pairs"], s["wts"], color, dout, torch.float64)
    g32 = gref.grad_antialias(s["pos"], s["pairs"], s["wts"], color, dout, torch.float32)
    _check_gradient(f"antialias, C = {C}", got, g64, g32)
    assert not got[:, 2].any()
    on_edge = np.zeros(V, bool)
    on_edge[s["pairs"]["a"]] = True
    on_edge[s["pairs"]["b"]] = True
    assert on_edge.sum() > 20 and (~on_edge).sum() > 20
    assert not got[~on_edge].any()                                       # touches no silhouette pair: exactly 0
    assert (np.abs(got[on_edge]).sum(axis=1) > 0).sum() > 20


def _rows_centroid(mask):
    m = mask[..., 0].double()
    rows = torch.arange(m.shape[0], device=m.device, dtype=torch.float64)[:, None]
    cols = torch.arange(m.shape[1], device=m.device, dtype=torch.float64)[None, :]
    return float((m * rows).sum() / m.sum()), float((m * cols).sum() / m.sum())


@pytest.mark.parametrize("axis,shift", [(0, 1.5), (0, -1.5), (1, 1.5), (1, -1.5)])
def test_mask_loss_descends_towards_the_target(axis, shift):
    """A quad's antialiased mask against the mask of the same quad moved by ``shift`` pixels: the loss sum (mask -
    target)^2 falls when the quad moves towards the target, so sum_v dL/d(coordinate)_v has the sign opposite to the
    shift.  No reference gradient is involved.  x: column c has x_ndc = (2c + 1)/W - 1, growing with c, so a target moved
    to larger columns lies at larger clip x: expected sum_v dL/dx_v < 0.  y: by the header's convention row 0 is
    y_ndc = -1 and row r has y_ndc = (2r + 1)/H - 1, growing with r (no flip between array rows and clip y: the array is
    bottom-up in OpenGL's sense), so a target moved to larger ROWS lies at larger clip y: expected sum_v dL/dy_v < 0.  That
    the target did move to larger columns / rows is checked on the arrays themselves, by their centroids."""
    from garmentdreamer_amd import mesh_deform as md
    box = [20.3, 40.6, 14.2, 33.7]                                        # x0, x1, y0, y1 in pixels
    moved = list(box)
    moved[2 * axis] += shift
    moved[2 * axis + 1] += shift
    (pos, tri), (pos_t, _) = gref.quad_scene(H, W, *box), gref.quad_scene(H, W, *moved)
    tri_d = _dev(tri)

    def mask_of(p):
        rast = md.rasterize(p, tri_d, (H, W))
        return md.antialias(torch.clamp(rast[..., -1:], 0, 1).detach(), rast, p, tri_d)

    target = mask_of(_dev(pos_t))
    p = _dev(pos).requires_grad_(True)
    mask = mask_of(p)
    r0, c0 = _rows_centroid(mask.detach())
    r1, c1 = _rows_centroid(target)
    moved_by = (c1 - c0, r1 - r0)[axis]
    # along the axis by the shift; across it only by what the blend at the four corner pixels can differ (a corner pixel
    # receives from two neighbours; four pixels at ~10 pixels from the centroid over a mass of ~400: below 0.1)
    assert abs(moved_by - shift) < 0.1 and abs((r1 - r0, c1 - c0)[axis]) < 0.1
    ((mask - target) ** 2).sum().backward()
    total = float(p.grad[:, axis].double().sum())
    print("axis", axis, "shift", shift, "sum of dL/dcoordinate", total)
    assert total * shift < 0


def test_backwards_are_bit_reproducible():
    s = _scene("edge")
    rng = np.random.RandomState(6)
    attr = rng.uniform(-1, 1, size=(s["pos"].shape[0], 3)).astype(np.float32)
    color = rng.uniform(0, 1, size=(H, W, 3)).astype(np.float32)
    dout = rng.uniform(-1, 1, size=(H, W, 3)).astype(np.float32)
    for fn, x in ((_interpolate_rasterize_grad, attr), (_antialias_grad, color)):
        first, second = fn("edge", x, dout), fn("edge", x, dout)
        assert first.abs().max() > 0 and torch.equal(first.view(torch.int32), second.view(torch.int32))
    # the gradient to rast on its own
    from garmentdreamer_amd import mesh_deform as md
    pos, tri, topo = _gpu_scene("edge")
    grads = []
    for _ in range(2):
        rast = md.rasterize(pos, tri, (H, W)).requires_grad_(True)
        md.interpolate(_dev(attr), rast, tri, pos, topo).backward(_dev(dout))
        grads.append(rast.grad)
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))
    g = grads[0].cpu().numpy()
    assert not g[..., 2:].any() and not g[s["rast"][..., 3] == 0].any() and np.abs(g[..., :2]).max() > 0
    a = attr[s["tri"][np.maximum(s["rast"][..., 3].astype(int) - 1, 0)]].astype(np.float64)     # [H,W,3 corners,C]
    want = np.stack(((dout * (a[:, :, 0] - a[:, :, 2])).sum(-1), (dout * (a[:, :, 1] - a[:, :, 2])).sum(-1)), -1)
    want[s["rast"][..., 3] == 0] = 0
    assert np.abs(g[..., :2] - want).max() <= 1e-5                       # three products of values <= 2 in fp32


def test_both_modules_give_bit_equal_gradients_where_both_have_one():
    """``mesh_render`` and ``mesh_deform`` are two policies over the same ops: with the same attr / colour, upstream
    gradient, rast, pos and topology, the gradient to ``attr`` of ``interpolate`` and, with ``pos`` detached, the gradient
    to ``color`` of ``antialias`` are the same bits.  Neither backward uses atomics, so no tolerance is involved."""
    from garmentdreamer_amd import mesh_deform as md
    from garmentdreamer_amd import mesh_render as mr
    pos, tri, topo = _gpu_scene("edge")
    rast = mr.rasterize(pos, tri, (H, W))
    rng = np.random.RandomState(40)

    def grad_of(op, x, dout):
        x = x.clone().requires_grad_(True)
        op(x).backward(dout)
        return x.grad

    for C in (1, 3, 8):
        attr = _dev(rng.uniform(-1, 1, size=(pos.shape[0], C)).astype(np.float32))
        dout = _dev(rng.uniform(-1, 1, size=(H, W, C)).astype(np.float32))
        fixed = grad_of(lambda a: mr.interpolate(a, rast, tri, pos=pos, topology=topo), attr, dout)
        moving = grad_of(lambda a: md.interpolate(a, rast, tri, pos, topo), attr, dout)
        assert tuple(fixed.shape) == (pos.shape[0], C) and fixed.abs().max() > 0, C
        assert torch.equal(fixed.view(torch.int32), moving.view(torch.int32)), C
    for C in (1, 3):
        color = _dev(rng.uniform(0, 1, size=(H, W, C)).astype(np.float32))
        dout = _dev(rng.uniform(-1, 1, size=(H, W, C)).astype(np.float32))
        fixed = grad_of(lambda c: mr.antialias(c, rast, pos, tri, topology=topo), color, dout)
        moving = grad_of(lambda c: md.antialias(c, rast, pos.detach(), tri, topo), color, dout)
        assert fixed.abs().max() > 0 and not torch.equal(fixed, dout), C      # the blend did something
        assert torch.equal(fixed.view(torch.int32), moving.view(torch.int32)), C


def test_visible_vertices():
    from garmentdreamer_amd import mesh_deform as md
    s = _scene("edge")
    pos, tri, _ = _gpu_scene("edge")
    V = pos.shape[0]

    def visible(rast):
        ids = np.unique(rast[..., 3].astype(int))
        want = np.zeros(V, bool)
        want[s["tri"][ids[ids > 0] - 1].ravel()] = True
        return want

    rast = md.rasterize(pos, tri, (H, W))
    vis = md.visible_vertices(rast, tri, V)
    assert vis.dtype == torch.bool and tuple(vis.shape) == (V,)
    want = visible(s["rast"])
    assert 10 < want.sum() < V - 10
    np.testing.assert_array_equal(vis.cpu().numpy(), want)
    # a second view (the scene mirrored in x, at another resolution) accumulates the union
    other = md.rasterize(pos * _dev(np.array([-1, 1, 1, 1], np.float32)), tri, (40, 56))
    want2 = visible(other.cpu().numpy())
    assert (want2 & ~want).any() and (want & ~want2).any()
    np.testing.assert_array_equal(md.visible_vertices([rast, other[None]], tri, V).cpu().numpy(), want | want2)


def test_gbuffer_renderer():
    from garmentdreamer_amd import mesh_deform as md
    from garmentdreamer_amd import mesh_render as mr
    v, tri, vn = scenes.tube()
    mvp = scenes.perspective(scenes.FOVY) @ np.linalg.inv(scenes.look_at_pose(scenes.CAMPOS))
    mvps = [_dev(mvp.astype(np.float32)), _dev((mvp @ np.diag([-1.0, 1, 1, 1])).astype(np.float32))]
    tri_d = _dev(tri)
    renderer = md.GBufferRenderer(near=0.01, far=100)
    verts, normals = _dev(v).requires_grad_(True), _dev(vn).requires_grad_(True)
    out = renderer.render(mvps, verts, tri_d.long(), normals, (H, W), ["mask", "position", "normal"])
    assert len(out) == 2 and all(sorted(g) == ["mask", "normal", "position"] for g in out)
    topo = mr.build_topology(tri_d, num_vertices=v.shape[0])
    for g, m in zip(out, mvps):
        pos = md.GBufferRenderer.transform_pos(m, verts.detach())
        rast = mr.rasterize(pos, tri_d, (H, W))
        assert 0.05 < (rast[..., 3] > 0).float().mean() < 0.9
        by_hand = dict(mask=torch.clamp(rast[..., -1:], 0, 1), position=mr.interpolate(verts.detach(), rast, tri_d),
                       normal=mr.interpolate(normals.detach(), rast, tri_d))
        for k, x in by_hand.items():
            assert tuple(g[k].shape) == (H, W, x.shape[-1])
            assert torch.equal(g[k].detach(), mr.antialias(x.contiguous(), rast, pos, tri_d, topology=topo)), k
    target = _dev(np.random.RandomState(8).uniform(0, 1, size=(H, W, 3)).astype(np.float32))
    loss = sum(((g["mask"] - 0.5) ** 2).sum() + ((g["position"] - target) ** 2).sum() + ((g["normal"] - target) ** 2).sum()
               for g in out)
    loss.backward()
    for t in (verts, normals):
        assert tuple(t.grad.shape) == tuple(t.shape) and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0
    # without antialiasing the mask is piecewise constant: a zero gradient; the position channel still has one
    verts2 = _dev(v).requires_grad_(True)
    plain = renderer.render(mvps[0], verts2, tri_d, None, (H, W), ["mask", "position"], with_antialiasing=False)[0]
    assert torch.equal(plain["mask"].detach(), torch.clamp(mr.rasterize(
        md.GBufferRenderer.transform_pos(mvps[0], verts2.detach()), tri_d, (H, W))[..., -1:], 0, 1))
    (g_mask,) = torch.autograd.grad(((plain["mask"] - 0.5) ** 2).sum(), verts2, retain_graph=True)
    (g_pos,) = torch.autograd.grad(((plain["position"] - target) ** 2).sum(), verts2)
    assert not g_mask.any() and g_pos.abs().max() > 0 and torch.isfinite(g_pos).all()
    # visibility: the 8x upsampled id images of both views
    vis = renderer.vertex_visibility(mvps, verts, tri_d, (H, W), upsample=8)
    rasts = [mr.rasterize(md.GBufferRenderer.transform_pos(m, verts.detach()), tri_d, (8 * H, 8 * W)) for m in mvps]
    ids = torch.unique(torch.cat([r[..., 3].long().flatten() for r in rasts]))
    want = torch.zeros(v.shape[0], dtype=torch.bool, device=DEV)
    want[torch.unique(tri_d[ids[ids > 0] - 1].long())] = True
    assert torch.equal(vis, want) and 10 < int(want.sum()) < v.shape[0]


def test_documented_errors():
    from garmentdreamer_amd import mesh_deform as md
    from garmentdreamer_amd import mesh_render as mr
    pos, tri, topo = _gpu_scene("edge")
    moving = pos.clone().requires_grad_(True)
    rast = md.rasterize(pos, tri, (H, W))
    color = torch.zeros(H, W, 3, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU path"):
        md.rasterize(moving.cpu(), tri, (H, W))
    with pytest.raises(RuntimeError, match="no CPU path"):
        md.antialias(color.cpu(), rast, moving, tri, topo)
    with pytest.raises(RuntimeError, match="no CPU path"):
        md.interpolate(pos[:, :3].contiguous(), rast.cpu(), tri, moving, topo)
    with pytest.raises(ValueError, match="minibatch"):
        md.rasterize(moving[None].repeat(2, 1, 1), tri, (H, W))
    with pytest.raises(ValueError, match="minibatch"):
        md.antialias(color[None].repeat(2, 1, 1, 1), rast, moving, tri, topo)
    with pytest.raises(ValueError, match="minibatch"):
        md.visible_vertices(rast[None].repeat(2, 1, 1, 1), tri, pos.shape[0])
    other = mr.build_topology(tri[:-1], num_vertices=pos.shape[0])       # another mesh's topology
    with pytest.raises(ValueError, match="topology"):
        md.rasterize(moving, tri, (H, W), other)
    with pytest.raises(ValueError, match="topology"):
        md.interpolate(pos[:, :3].contiguous().requires_grad_(True), rast, tri, moving, other)
    with pytest.raises(ValueError, match="topology"):
        md.antialias(color, rast, moving, tri, other)
    with pytest.raises(ValueError, match="topology"):
        md.rasterize(moving, tri, (H, W), mr.build_topology(tri.cpu(), num_vertices=pos.shape[0]))
    with pytest.raises(TypeError, match="float32"):
        md.rasterize(moving.double(), tri, (H, W))
    with pytest.raises(ValueError, match="channels"):
        md.interpolate(torch.zeros(pos.shape[0], 9, device=DEV), rast, tri, moving)
