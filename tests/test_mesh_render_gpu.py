"""GPU parity of the mesh render path (csrc/raster_mesh.hip, garmentdreamer_amd/mesh_render.py) against the numpy
statement of its definitions (tests/mesh_reference.py): ``rast`` and the antialias weights bit for bit, interpolate and
the antialias blend within fp32 rounding, the two gradients against float64 sums, and ``MeshRenderer.render`` with its
gradient to a small MLP against the same pipeline assembled on the CPU from the reference's ``rast`` and ``wts``.

Scenes (tests/mesh_scenes.py): the generated open tube of tests/test_template_gpu.py (576 triangles) seen from above its
rim, plus hand-placed clip-space triangles for the rasterizer's edge cases."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_reference as ref
from tests import mesh_scenes as scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 48, 64                 # the issue's 64 x 48: not square, 48 rows; 3072 pixels = 12 workgroups


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _edge_scene():
    """The 64 x 48 scene and everything the reference says about it; shared and treated as read-only."""
    pos, tri, names = scenes.edge_case_scene()
    rast = ref.rasterize(pos, tri, H, W)
    opp = ref.build_opposite(tri)
    info = {}
    wts = ref.antialias_weights(rast, pos, tri, opp, info)
    return dict(pos=pos, tri=tri, names=names, rast=rast, opp=opp, wts=wts, info=info)


@functools.lru_cache(maxsize=None)
def _gpu_edge_scene():
    from garmentdreamer_amd import mesh_render as mr
    s = _edge_scene()
    pos, tri = _dev(s["pos"]), _dev(s["tri"])
    topo = mr.build_topology(tri, num_vertices=pos.shape[0])
    return pos, tri, topo, mr.rasterize(pos, tri, (H, W))


def test_rasterize_edge_cases_bit_exact():
    from garmentdreamer_amd import mesh_render as mr
    s = _edge_scene()
    pos, tri, _, rast = _gpu_edge_scene()
    assert rast.shape == (H, W, 4) and rast.dtype == torch.float32
    out = rast.cpu().numpy()
    np.testing.assert_array_equal(out[..., 3], s["rast"][..., 3])
    np.testing.assert_array_equal(_bits(out), _bits(s["rast"]))
    # the scene does what it is there for
    ids = s["rast"][..., 3].astype(int) - 1
    n = s["names"]
    assert (ids == n["large_a"]).sum() > 256 and (ids == n["large_b"]).sum() > 256      # the one-wave-per-triangle path
    assert (ids == n["dup_0"]).any() and not (ids == n["dup_1"]).any()                   # a tie goes to the lowest id
    assert all(not (ids == n[k]).any() for k in ("zero_area", "behind", "w_zero", "wholly_out"))
    assert (ids == n["partly_out"]).any() and (ids == n["z_range"]).any() and (ids == n["w_varies"]).any()
    assert ((ids >= 0) & (ids < 576)).sum() > 300 and (ids < 0).sum() > 300
    # a second run returns the same bits; a minibatch axis is carried through
    again = mr.rasterize(pos[None], tri, (H, W))
    assert again.shape == (1, H, W, 4) and torch.equal(again[0].view(torch.int32), rast.view(torch.int32))


def test_rasterize_micro_triangles_512_bit_exact():
    """20 736 triangles of a few pixels each at 512 x 512: the workload's density."""
    from garmentdreamer_amd import mesh_render as mr
    pos, tri = scenes.tube_clip(96, 108)
    assert tri.shape[0] >= 20000
    want = ref.rasterize(pos, tri, 512, 512, window=16)
    assert 0.2 < (want[..., 3] > 0).mean() < 0.6
    out = mr.rasterize(_dev(pos), _dev(tri), (512, 512))
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want))
    assert torch.equal(mr.rasterize(_dev(pos), _dev(tri), (512, 512)).view(torch.int32), out.view(torch.int32))


def test_rasterize_empty_and_degenerate_inputs():
    from garmentdreamer_amd import mesh_render as mr
    pos = _dev(np.array([[0, 0, 0, 1], [np.nan, 0, 0, 1], [0, np.inf, 0, 1], [1e30, 0, 0, 1e-30]], dtype=np.float32))
    for tri in (np.zeros((0, 3), np.int32), np.array([[0, 1, 2], [0, 2, 3], [0, 0, 0]], np.int32)):
        assert not mr.rasterize(pos, _dev(tri), (5, 7)).any()


@pytest.mark.parametrize("C", [1, 3, 8])
def test_interpolate_forward_and_backward(C):
    from garmentdreamer_amd import mesh_render as mr
    s = _edge_scene()
    pos, tri, topo, rast = _gpu_edge_scene()
    V = pos.shape[0]
    rng = np.random.RandomState(C)
    attr = rng.uniform(-1, 1, size=(V, C)).astype(np.float32)
    a = _dev(attr).requires_grad_(True)
    out = mr.interpolate(a, rast, tri, pos=pos, topology=topo)
    assert out.shape == (H, W, C)
    want = ref.interpolate(attr, s["rast"], s["tri"])
    err = np.abs(out.detach().cpu().numpy() - want).max()
    print("interpolate forward max abs error", err)
    assert err <= 1e-6
    assert not out.detach()[_dev(s["rast"][..., 3] == 0)].any()
    # backward against a float64 sum of the same terms: n * 2^-24 for the few hundred terms a vertex collects
    g = rng.uniform(-1, 1, size=(H, W, C)).astype(np.float32)
    out.backward(_dev(g))
    total, mag = ref.interpolate_backward_terms(g, s["rast"], s["tri"], V)
    got = a.grad.cpu().numpy()
    print("interpolate backward max error / bound", (np.abs(got - total) / np.maximum(1e-5 * mag, 1e-30)).max())
    assert np.all(np.abs(got - total) <= 1e-5 * mag)
    seen = np.zeros(V, bool)
    seen[s["tri"][np.unique(s["rast"][..., 3].astype(int))[1:] - 1].ravel()] = True
    assert (~seen).sum() > 10 and not got[~seen].any()                               # exactly zero, every element written
    assert np.abs(got[seen]).sum() > 0
    # bit-identical on a second run
    a2 = _dev(attr).requires_grad_(True)
    mr.interpolate(a2, rast, tri, pos=pos).backward(_dev(g))                         # topology built on the fly
    assert torch.equal(a2.grad.view(torch.int32), a.grad.view(torch.int32))
    # the op is linear in attr: <J d, g> = <d, J^T g>
    d = rng.uniform(-1, 1, size=(V, C)).astype(np.float32)
    lhs = (mr.interpolate(_dev(d), rast, tri).double() * _dev(g).double()).sum().item()
    rhs = (_dev(d).double() * a.grad.double()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * (mag * np.abs(d)).sum()


def test_interpolate_needs_pos_for_the_gradient_and_limits_channels():
    from garmentdreamer_amd import mesh_render as mr
    pos, tri, _, rast = _gpu_edge_scene()
    with pytest.raises(RuntimeError, match="needs pos="):
        mr.interpolate(torch.zeros(pos.shape[0], 3, device=DEV, requires_grad=True), rast, tri)
    with pytest.raises(ValueError, match="channels"):
        mr.interpolate(torch.zeros(pos.shape[0], 9, device=DEV), rast, tri)


def test_antialias_weights_bit_exact():
    from garmentdreamer_amd import mesh_render as mr
    s = _edge_scene()
    pos, tri, topo, rast = _gpu_edge_scene()
    np.testing.assert_array_equal(topo.opp.cpu().numpy(), s["opp"])
    info = s["info"]
    assert (s["wts"] != 0).sum() >= 50, info
    assert min(info["to_outer"], info["to_inner"], info["horizontal"], info["vertical"], info["fold"],
               info["boundary"]) >= 1, info
    wts = mr.antialias_weights(rast, pos, tri, topo)
    np.testing.assert_array_equal(_bits(wts.cpu().numpy()), _bits(s["wts"]))
    assert torch.equal(mr.antialias_weights(rast, pos, tri, topo).view(torch.int32), wts.view(torch.int32))


@pytest.mark.parametrize("C", [1, 3])
def test_antialias_apply_adjoint_and_interior(C):
    from garmentdreamer_amd import mesh_render as mr
    s = _edge_scene()
    pos, tri, topo, rast = _gpu_edge_scene()
    rng = np.random.RandomState(10 + C)
    x = rng.uniform(0, 1, size=(H, W, C)).astype(np.float32)
    y = rng.uniform(0, 1, size=(H, W, C)).astype(np.float32)
    xg = _dev(x).requires_grad_(True)
    out = mr.antialias(xg, rast, pos, tri, topology=topo)
    want = ref.antialias_apply(x, s["wts"])
    err = np.abs(out.detach().cpu().numpy() - want).max()
    print("antialias apply max abs error", err)
    assert err <= 1e-6
    # shared weights give the same bits as the analysis inside the call, and as the topology built on the fly
    wts = mr.antialias_weights(rast, pos, tri, topo)
    assert torch.equal(mr.antialias(_dev(x), rast, pos, tri, weights=wts), out.detach())
    assert torch.equal(mr.antialias(_dev(x)[None], rast, pos, tri)[0], out.detach())
    # pixels whose four neighbours lie on the same triangle are unchanged bit for bit
    ids = s["rast"][..., 3]
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = ((ids[1:-1, 1:-1] == ids[1:-1, :-2]) & (ids[1:-1, 1:-1] == ids[1:-1, 2:]) &
                         (ids[1:-1, 1:-1] == ids[:-2, 1:-1]) & (ids[1:-1, 1:-1] == ids[2:, 1:-1]))
    assert inner.sum() > 500
    np.testing.assert_array_equal(_bits(out.detach().cpu().numpy()[inner]), _bits(x[inner]))
    assert (out.detach().cpu().numpy() != x).sum() > 50
    # <apply(x), y> = <x, adjoint(y)>
    out.backward(_dev(y))
    adj = xg.grad
    lhs = (out.detach().double() * _dev(y).double()).sum().item()
    rhs = (_dev(x).double() * adj.double()).sum().item()
    print("adjoint identity relative difference", abs(lhs - rhs) / abs(lhs))
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)
    assert np.abs(adj.cpu().numpy() - ref.antialias_adjoint(y, s["wts"])).max() <= 1e-6


def _mlp(device):
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(3, 16), torch.nn.ReLU(), torch.nn.Linear(16, 3), torch.nn.Sigmoid())
    return net.to(device)


def _t_apply(x, wts):
    """mesh_reference.antialias_apply in differentiable CPU torch."""
    z = torch.zeros_like(x)
    nbs = [torch.cat((z[:, :1], x[:, :-1]), 1), torch.cat((x[:, 1:], z[:, :1]), 1),
           torch.cat((z[:1], x[:-1]), 0), torch.cat((x[1:], z[:1]), 0)]
    acc = x
    for k, nb in enumerate(nbs):
        acc = acc + wts[..., k:k + 1] * (nb - x)
    return acc


def _reference_render(v, tri, vn, net, pose, pos, v_cam, h, w):
    """The renderer's pipeline on the CPU, from the numpy reference's rast and wts of the clip-space positions ``pos``."""
    rast = ref.rasterize(pos, tri, h, w)
    wts = torch.from_numpy(ref.antialias_weights(rast, pos, tri, ref.build_opposite(tri)))
    tr = torch.from_numpy(rast)
    alpha = _t_apply(tr[..., 3:].clamp(0, 1), wts).clamp(0, 1)
    depth = torch.from_numpy(ref.interpolate(-v_cam[:, [2]], rast, tri))
    xyz = torch.from_numpy(ref.interpolate(v, rast, tri))
    mask = (alpha > 0).view(-1)
    color = torch.zeros(h * w, 3)
    color[mask] = net(xyz.view(-1, 3)[mask])
    color = _t_apply(color.view(h, w, 3), wts).clamp(0, 1)
    image = alpha * color + (1 - alpha) * 1.0
    n_ = torch.from_numpy(ref.interpolate(vn, rast, tri))
    normal = n_ / torch.sqrt(torch.clamp((n_ * n_).sum(-1, keepdim=True), min=1e-20))
    with torch.no_grad():
        view = torch.nn.functional.normalize(_t_apply(xyz, wts) - torch.from_numpy(pose[:3, 3]), dim=-1)
        cosv = torch.nn.functional.cosine_similarity(view, _t_apply(n_, wts), dim=-1, eps=1e-6)
    return dict(image=image, alpha=alpha, depth=depth, normal=(normal + 1) / 2, cosinesview=cosv), rast


def test_mesh_renderer_outputs_and_mlp_gradients():
    from garmentdreamer_amd import mesh_render as mr
    v, tri, vn = scenes.tube()
    pose, proj = scenes.look_at_pose(scenes.CAMPOS), mr.perspective(scenes.FOVY)
    h = w = 64
    cpu_net, gpu_net = _mlp("cpu"), _mlp(DEV)
    renderer = mr.MeshRenderer(_dev(v), _dev(tri), _dev(vn), gpu_net)
    # the two 4 x 4 products that make v_clip are torch's; the reference starts from THEIR bits (a last-bit difference
    # in a position can move a snapped vertex by 1/256 pixel), after a check that they are the right positions
    v_cam, pos = (t.cpu().numpy() for t in renderer.clip_positions(pose, proj))
    want_pos, want_cam = scenes.clip_positions(v, pose, proj)
    assert np.allclose(pos, want_pos, rtol=1e-5, atol=1e-6) and np.allclose(v_cam, want_cam, rtol=1e-5, atol=1e-6)
    want, rast = _reference_render(v, tri, vn, cpu_net, pose, pos, v_cam, h, w)
    out = renderer.render(pose, proj, h, w)
    assert sorted(out) == ["alpha", "cosinesview", "depth", "image", "normal"]
    assert 0.1 < (rast[..., 3] > 0).mean() < 0.9
    shapes = dict(image=(h, w, 3), alpha=(h, w, 1), depth=(h, w, 1), normal=(h, w, 3), cosinesview=(h, w))
    # 1e-5 absolute for all five: a handful of fp32 roundings (2^-24 each) of values no larger than the depth, about 2
    tol = dict(image=1e-5, alpha=1e-5, depth=1e-5, normal=1e-5, cosinesview=1e-5)
    for k in shapes:
        assert tuple(out[k].shape) == shapes[k], k
        err = (out[k].detach().cpu() - want[k].detach()).abs().max().item()
        print(k, "max abs error", err)
        assert err <= tol[k], (k, err)
    target = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, size=(h, w, 3)).astype(np.float32))
    ((out["image"] - target.to(DEV)) ** 2).mean().backward()
    ((want["image"] - target) ** 2).mean().backward()
    for pg, pc in zip(gpu_net.parameters(), cpu_net.parameters()):
        assert pc.grad.abs().max() > 0
        err = (pg.grad.cpu() - pc.grad).abs().max().item()
        print("parameter gradient", tuple(pc.shape), "max abs error", err, "scale", pc.grad.abs().max().item())
        assert torch.allclose(pg.grad.cpu(), pc.grad, rtol=1e-4, atol=1e-4 * pc.grad.abs().max().item())
    # a second render returns the same bits
    again = renderer.render(pose, proj, h, w)
    assert all(torch.equal(again[k], out[k]) for k in shapes)


def test_documented_errors():
    from garmentdreamer_amd import mesh_render as mr
    v, tri, vn = scenes.tube()
    pos, tri_d, _, rast = _gpu_edge_scene()
    moving = pos.clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="vertex positions"):
        mr.rasterize(moving, tri_d, (H, W))
    with pytest.raises(NotImplementedError, match="vertex positions"):
        mr.antialias(torch.zeros(H, W, 3, device=DEV), rast, moving, tri_d)
    with pytest.raises(NotImplementedError, match="vertex positions"):
        mr.interpolate(torch.zeros(pos.shape[0], 3, device=DEV), rast, tri_d, pos=moving)
    with pytest.raises(NotImplementedError, match="vertex positions"):
        mr.MeshRenderer(_dev(v).requires_grad_(True), _dev(tri), _dev(vn), lambda x: x)
    renderer = mr.MeshRenderer(_dev(v), _dev(tri), _dev(vn), lambda x: torch.full_like(x, 0.5))
    with pytest.raises(ValueError, match="ssaa"):
        renderer.render(scenes.look_at_pose(scenes.CAMPOS), mr.perspective(scenes.FOVY), 32, 32, ssaa=2)
    with pytest.raises(ValueError, match="minibatch"):
        mr.rasterize(pos[None].repeat(2, 1, 1), tri_d, (H, W))
