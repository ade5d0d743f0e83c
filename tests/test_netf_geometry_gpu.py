"""GPU checks of the NeTF stage with free geometry (garmentdreamer_amd/netf_geometry.py): ``DeformableNeTFRenderer`` against
``NeTFRenderer`` at zero offsets, the plumbing of the field's position gradient into ``v_offsets.grad``, that gradient
against the float64 CPU statement (tests/texture_position_reference.py), the three-range optimizer against
``torch.optim.Adam`` in float64, and ``remesh``.  The mesh is an icosphere (42 vertices / 80 faces; 162 / 320 for
``remesh``) rendered at 64 x 64; the field has the layout ``grid_layout(16, 2, 1.3, 10)``."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_scenes as scenes
from tests import texture_position_reference as pref
from tests import texture_reference as tref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = W = 64
KW = dict(num_levels=16, base_resolution=2, per_level_scale=1.3, log2_hashmap_size=10)
PARAMS = ("grid", "w1", "b1", "w2", "b2")


def icosphere(subdivisions, radius=0.35, center=(0.0, 0.0, 0.5)):
    """(vertices float32 [V,3], triangles int32 [F,3]): 12 / 20, 42 / 80, 162 / 320, ..., outward orientation"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1),
         (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return (np.array(v) * radius + np.array(center)).astype(np.float32), np.array(f, dtype=np.int32)


def _camera():
    from garmentdreamer_amd import mesh_render as mr
    return scenes.look_at_pose(scenes.CAMPOS), mr.perspective(scenes.FOVY)


@functools.lru_cache(maxsize=None)
def _params():
    lay = tref.layout(**KW)
    g = torch.Generator().manual_seed(21)
    rnd = lambda *shape, s=1.0: ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * s).float()
    return lay, dict(grid=rnd(int(lay["offset"][-1]) * 2), w1=rnd(32, 32, s=0.3), b1=rnd(32, s=0.3), w2=rnd(3, 32, s=0.3),
                     b2=rnd(3, s=0.3))


def _field(position_gradient=True):
    from garmentdreamer_amd import texture_field as tf
    _, p = _params()
    fld = tf.TextureField(tf.HashGridEncoder.from_layout(tf.grid_layout(**KW)), position_gradient=position_gradient).to(DEV)
    with torch.no_grad():
        fld.encoder.params.copy_(p["grid"])
        for dst, k in zip(fld.mlp.parameters(), PARAMS[1:]):
            dst.copy_(p[k])
    return fld


def _renderer(subdivisions=1, texture_fn=None):
    from garmentdreamer_amd import netf_geometry as ng
    v, f = icosphere(subdivisions)
    return ng.DeformableNeTFRenderer(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV),
                                     _field() if texture_fn is None else texture_fn)


def _target():
    return torch.from_numpy(np.random.RandomState(5).uniform(0, 1, size=(H, W, 3)).astype(np.float32)).to(DEV)


def _loss(out, target):
    return ((out["image"] - target) ** 2).sum() + 0.3 * out["alpha"].sum() + 0.1 * out["depth"].sum()


def test_icosphere_sizes():
    for s, (nv, nf) in enumerate(((12, 20), (42, 80), (162, 320))):
        v, f = icosphere(s)
        assert v.shape == (nv, 3) and f.shape == (nf, 3)


def test_zero_offsets_render_bit_equal_to_netf_renderer():
    from garmentdreamer_amd import texture_field as tf
    r = _renderer()
    assert isinstance(r, tf.NeTFRenderer) and isinstance(r.v_offsets, torch.nn.Parameter) and not r.v_offsets.any()
    assert torch.equal(r.v.detach(), r.base_v) and r.v.requires_grad
    fixed = tf.NeTFRenderer(r.base_v, r.f, r.vertex_normals(), r.texture_fn)
    pose, proj = _camera()
    a, b = r.render(pose, proj, H, W), fixed.render(pose, proj, H, W)
    for k in ("image", "alpha", "depth", "cosinesview", "normal"):
        assert torch.equal(a[k].detach(), b[k].detach()), k
    assert 0.05 < float((a["alpha"] > 0).float().mean()) < 0.9
    assert a["image"].requires_grad and a["alpha"].requires_grad and a["depth"].requires_grad
    assert not a["normal"].requires_grad and not a["cosinesview"].requires_grad
    with pytest.raises(ValueError, match="ssaa"):
        r.render(pose, proj, H, W, ssaa=2)
    from garmentdreamer_amd import netf_geometry as ng
    with pytest.raises(ValueError, match="position_gradient"):
        ng.DeformableNeTFRenderer(r.base_v, r.f, _field(position_gradient=False))


def test_vertex_normals_are_the_reference_s_formula():
    """the sum of the unit face normals by scatter_add in float64 (mesh_renderer.py:385-396); the float32 gather is within
    a few roundings of a sum of at most six unit vectors"""
    r = _renderer()
    v, f = r.base_v.cpu().double(), r.f.cpu().long()
    fn = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=-1)
    fn = fn / fn.norm(dim=1, keepdim=True)
    want = torch.zeros_like(v)
    for i in range(3):
        want.index_add_(0, f[:, i], fn)
    got = r.vertex_normals()
    assert float((got.cpu().double() - want).abs().max()) <= 16 * 2.0 ** -24 * 6
    assert float(got.norm(dim=1).min()) > 3.0                                  # a sum, not normalised
    assert torch.equal(got, r.vertex_normals()) and not got.requires_grad     # no atomics: reruns bit-identical


class _Recorder:
    """texture_fn that keeps what it was given, what it returned, and the gradients of both"""

    def __init__(self, fn):
        self.fn = fn

    def __call__(self, x, mask):
        self.x, self.mask = x, mask.detach()
        x.retain_grad()
        self.out = self.fn(x, mask)
        self.out.retain_grad()
        return self.out


class _Replay(torch.autograd.Function):
    """stands in for the field: returns the recorded colour, and the recorded dx whatever it is handed"""

    @staticmethod
    def forward(ctx, x, color, dx):
        ctx.save_for_backward(dx)
        return color.clone()

    @staticmethod
    def backward(ctx, dcolor):
        return ctx.saved_tensors[0], None, None


@functools.lru_cache(maxsize=None)
def _recorded_backward():
    """one render and backward through a recording field: (renderer, recorder, v_offsets.grad, visible vertices)"""
    from garmentdreamer_amd import mesh_deform as md
    rec = _Recorder(_field())
    r = _renderer(texture_fn=rec)
    pose, proj = _camera()
    out = r.render(pose, proj, H, W)
    _loss(out, _target()).backward()
    with torch.no_grad():
        _, v_clip = r._clip_of(r.v, r._matrices(pose, proj))
        visible = md.visible_vertices(md.rasterize(v_clip, r.f, (H, W)), r.f, r.base_v.shape[0])
    return r, rec, r.v_offsets.grad.clone(), visible


def test_position_gradient_reaches_the_offsets_unchanged():
    r, rec, grad, _ = _recorded_backward()
    color, dx = rec.out.detach(), rec.x.grad.detach()
    assert dx.any()
    replay = _renderer(texture_fn=lambda x, mask: _Replay.apply(x, color, dx))
    pose, proj = _camera()
    _loss(replay.render(pose, proj, H, W), _target()).backward()
    assert torch.equal(replay.v_offsets.grad, grad)
    # and it matters: without dx the offsets get another gradient
    blind = _renderer(texture_fn=lambda x, mask: _Replay.apply(x, color, torch.zeros_like(dx)))
    _loss(blind.render(pose, proj, H, W), _target()).backward()
    assert not torch.equal(blind.v_offsets.grad, grad)


def test_recorded_dx_against_float64():
    """the rule of tests/test_texture_position_gpu.py at the points the render sampled.  Measured on one MI355X: 766
    covered pixels, gpu 0.0204, float32 statement 0.0204 (a pixel's point within a float32 rounding of a cell wall falls
    into the neighbouring cell in float64, where the slope is another; the GPU and the float32 statement agree)."""
    _, rec, _, _ = _recorded_backward()
    lay, p = _params()
    p64 = {k: v.double() for k, v in p.items()}
    x, mask, dcolor = rec.x.detach().cpu(), rec.mask.cpu().view(torch.uint8), rec.out.grad.cpu()
    want = pref.field_position_gradient(x, p64, lay, dcolor, mask)
    ref32 = pref.rel(pref.field_position_gradient(x, p, lay, dcolor, mask), want)
    err = pref.rel(rec.x.grad, want)
    print(f"recorded dx ({int((mask != 0).sum())} covered pixels): gpu {err:.3g} float32 statement {ref32:.3g} "
          f"allowed {4 * ref32:.3g}")
    assert err <= 4 * ref32
    assert not rec.x.grad.cpu()[mask == 0].any()


def test_offsets_gradient_is_there_where_the_mesh_shows_and_nowhere_else():
    _, _, grad, visible = _recorded_backward()
    assert torch.isfinite(grad).all()
    assert 5 < int(visible.sum()) < visible.numel() - 5                      # a front and a back
    assert bool(grad[visible].any(dim=1).all())                              # every visible vertex moves
    assert not grad[~visible].any()                                           # exactly zero behind


def test_optimizer_three_steps_against_float64_adam():
    """each step against ``torch.optim.Adam`` in float64 from the same parameters and the same gradients (its moments are
    its own, float64, over the three steps), to the tolerance of the texture optimizer's test: a dozen fp32 operations at
    2^-24 each on the step (2e-6 of it) and the rounding of the subtraction from p itself"""
    r = _renderer()
    fld = r.texture_fn
    lrs = (0.01, 0.001, 0.0001)
    groups = r.get_params(*lrs)
    assert [g["lr"] for g in groups] == list(lrs) and groups[2]["params"][0] is r.v_offsets
    assert groups[0]["params"][0] is fld.encoder.params and len(groups[1]["params"]) == 4
    opt = r.optimizer(*lrs)
    params = [fld.encoder.params] + list(fld.mlp.parameters()) + [r.v_offsets]
    plr = [lrs[0]] + [lrs[1]] * 4 + [lrs[2]]
    assert all(p.grad is not None and not p.grad.any() for p in params)
    assert params[0].data_ptr() == opt._flat.data_ptr()
    ref = [p.detach().double().clone().requires_grad_(True) for p in params]
    adam = torch.optim.Adam([{"params": [q], "lr": lr} for q, lr in zip(ref, plr)], betas=(0.9, 0.999), eps=1e-8)
    pose, proj = _camera()
    target = _target()
    for step in range(3):
        opt.zero_grad()
        _loss(r.render(pose, proj, H, W), target).backward()
        before = [p.detach().clone() for p in params]
        with torch.no_grad():
            for q, p in zip(ref, params):
                q.copy_(p.detach().double())
                q.grad = p.grad.detach().double().clone()
        opt.step()
        adam.step()
        for name, p, p0, q, lr in zip(PARAMS + ("v_offsets",), params, before, ref, plr):
            tol = 2e-6 * lr + 2.0 ** -24 * p0.double().abs()
            worst = float(((p.detach().double() - q.detach()).abs() - tol).max())
            assert worst <= 0, (step, name, worst)
            assert not torch.equal(p.detach(), p0), (step, name)              # every range moved
    assert opt.step_count == 3


def test_render_backward_step_never_wait_for_the_gpu():
    r = _renderer()
    opt = r.optimizer()
    pose, proj = _camera()
    target = _target()

    def iteration():
        opt.zero_grad()
        loss = _loss(r.render(pose, proj, H, W), target)
        loss.backward()
        opt.step()
        return loss.detach()

    first = iteration()                       # loads the library and warms the allocators
    before = r.v_offsets.detach().clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = iteration()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(first) and torch.isfinite(second)
    assert not torch.equal(before, r.v_offsets.detach())                      # the step moved the vertices


def test_remesh(tmp_path):
    from garmentdreamer_amd import mesh_geometry
    r = _renderer(subdivisions=2)
    v, f = r.base_v, r.f.long()
    edges = torch.cat([v[f[:, i]] - v[f[:, (i + 1) % 3]] for i in range(3)]).norm(dim=1)
    old_offsets, old_faces = r.v_offsets, r.f.shape[0]
    with torch.no_grad():
        r.v_offsets += 0.01                                                   # the CURRENT vertices are remeshed
    report = r.remesh(remesh_size=0.5 * float(edges.mean()), decimate_target=400)
    assert old_faces == 320 and report["faces_before"] == 320 and report["repaired"] is False
    assert "decimate" in report and report["faces_after"] == r.f.shape[0] <= 400
    mesh_geometry.build_geometry(r.f, r.base_v.shape[0], DEV)                 # raises on a non-manifold mesh
    centre = torch.tensor([0.01, 0.01, 0.51], device=DEV)
    assert float(((r.base_v - centre).norm(dim=1) - 0.35).abs().max()) < 0.03   # still that sphere, where it was moved to
    assert r.v_offsets is not old_offsets and isinstance(r.v_offsets, torch.nn.Parameter) and r.v_offsets.requires_grad
    assert r.v_offsets.shape == r.base_v.shape and not r.v_offsets.any() and r.v_offsets.grad is None
    assert r.topology.corner_ptr.shape[0] == r.base_v.shape[0] + 1 and r.vertex_normals().shape == r.base_v.shape
    pose, proj = _camera()
    out = r.render(pose, proj, H, W)
    _loss(out, _target()).backward()
    assert torch.isfinite(out["image"]).all() and float((out["alpha"] > 0).float().mean()) > 0.05
    assert torch.isfinite(r.v_offsets.grad).all() and r.v_offsets.grad.any()
    with torch.no_grad():
        r.v_offsets += 0.02
    obj, _, _ = r.export_mesh(str(tmp_path / "moved.obj"), texture_resolution=256, padding=2)
    rows = [line.split()[1:] for line in open(obj) if line.startswith("v ")]
    written = torch.tensor([[float(a) for a in row] for row in rows], dtype=torch.float64)
    assert torch.equal(written, (r.base_v + r.v_offsets).detach().cpu().double())
    assert not torch.equal(written, r.base_v.cpu().double())
