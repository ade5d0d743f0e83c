"""GPU checks of the second stage's G-buffer losses (garmentdreamer_amd/mesh_losses.py, the entries of
include/gd_mesh_losses.h in csrc/raster_gbuffer_losses.hip) and of the deformer's second-stage iteration
(garmentdreamer_amd/deformer.py) against the float64 statement of tests/mesh_losses_reference.py.

Method: the kernels are fed SYNTHETIC G-buffers (mesh_losses_reference.make_case), so the GPU and the float64 statement
read the same bits.  Tolerance, as tests/test_mesh_geometry_gpu.py: the normalised error max|g - g64| / max|g64| of the
GPU may be four times that of the SAME reference evaluated in float32 on the CPU on the same input; for a scalar loss the
float32 reference's error is the largest over three summation orders.  Every figure is printed.

The terms have thresholds (cv at 0, ct at epsilon, the L1 kink, the hole sign at 0); a pixel that changes sides is a
discontinuity, not an error.  The generator keeps every pixel 1e-3 away from each of them; that the float32 and the float64
reference then select identical pixel sets is asserted before the GPU is compared, and no pixel is left out of a comparison.

Shapes, H x W: 1 x 1; 5 x 7 (less than a wave); 64 x 64 (a multiple of 256); 67 x 131 (not one; 35 partials); 300 x 300
(352 partials: more than the final pass has threads)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import mesh_losses_reference as lref
from tests import mesh_scenes as scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"1x1": (1, 1, 11), "5x7": (5, 7, 12), "64x64": (64, 64, 13), "67x131": (67, 131, 14), "300x300": (300, 300, 15)}
TERMS = ("enhanced", "plain", "hole")
BIT = {"enhanced": 1, "plain": 2, "hole": 4}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name):
    """Everything the CPU reference says about a shape; computed once, shared and treated as read-only."""
    case = lref.make_case(*SHAPES[name])
    out = {"case": case, "r64": {}, "r32": {}}
    s64, s32 = lref.selections(case, torch.float64), lref.selections(case, torch.float32)
    for k in s64:                                  # the condition under which the comparison below means anything
        assert np.array_equal(s64[k], s32[k]), (name, k)
    out["counts"] = {"plain": int(s64["plain"].sum()), "hole": int(s64["hole"].sum())}
    for dtype, key in ((torch.float64, "r64"), (torch.float32, "r32")):
        c = lref.tensors(case, dtype)
        for term in TERMS:
            _, dn, dp = lref.gradients(case, dtype, lref.LOSSES[term])
            out[key][term] = {"loss": lref.loss_in_three_orders(c, term), "dnormal": dn, "dposition": dp}
    return out


@functools.lru_cache(maxsize=None)
def _gpu_case(name):
    return {k: _dev(v) for k, v in _case(name)["case"].items()}


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _raw(g, terms, dloss=(1.0, 1.0, 1.0), epsilon=lref.EPSILON):
    """Both entries called directly with every output and the scratch pre-filled with NaN: (stats [6], dnormal, dposition)."""
    from garmentdreamer_amd import _native
    L = _native.lib()
    s = torch.cuda.current_stream(DEV).cuda_stream
    H, W = g["normal"].shape[:2]
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())                          # noqa: E731
    camera = torch.cat((g["R"].reshape(9), g["center"].reshape(3)))
    scratch = _nan(L.gd_mesh_gbuffer_losses_scratch_bytes(H * W) // 4)
    stats, dn, dp = _nan(6), _nan(H, W, 3), _nan(H, W, 3)
    ins = [p(g[k]) for k in ("normal", "position", "mask", "normal_rf", "position_rf", "mask_rf", "T", "tmask")] + [p(camera)]
    assert L.gd_mesh_gbuffer_losses_forward(s, H, W, terms, *ins, epsilon, p(stats), p(scratch)) == 0
    d = torch.tensor(dloss, dtype=torch.float32, device=DEV)
    assert L.gd_mesh_gbuffer_losses_backward(s, H, W, terms, *ins, epsilon, p(stats), p(d), p(dn), p(dp)) == 0
    return stats, dn, dp


def _one_hot(term, value=1.0):
    return tuple(value if t == term else 0.0 for t in TERMS)


def _check(what, got, r64, r32, floor=0.0):
    """The 4x rule of the module docstring; ``r64`` / ``r32`` arrays, or lists of scalars (the first is torch's own sum).
    ``floor``: the resolution to which ``r64`` itself is known, where that is not float64's (stated by the caller)."""
    if isinstance(r64, list):
        want = r64[0]
        e_gpu = abs(float(got) - want) / abs(want)
        e_f32 = max(abs(r - want) / abs(want) for r in r32)
    else:
        assert np.isfinite(got).all() and np.abs(r64).max() > 0
        e_gpu, e_f32 = lref.normalised_error(got, r64), lref.normalised_error(r32, r64)
    allowed = 4 * max(e_f32, floor)
    print(f"{what}: normalised error GPU {e_gpu:.3e}, float32 reference {e_f32:.3e}, allowed {allowed:.3e}")
    assert e_gpu <= allowed, (what, e_gpu, e_f32)


@pytest.mark.parametrize("name", list(SHAPES))
def test_each_term_alone_and_fused_against_the_float64_statement(name):
    c, g = _case(name), _gpu_case(name)
    fused_stats, fused_dn, fused_dp = _raw(g, 7)
    assert torch.isfinite(fused_stats[:4]).all() and torch.isfinite(fused_dn).all() and torch.isfinite(fused_dp).all()
    counts = fused_stats[4:].view(torch.int32).tolist()
    assert counts == [c["counts"]["plain"], c["counts"]["hole"]]
    for k, term in enumerate(TERMS):
        runs = [_raw(g, BIT[term], _one_hot(term)) for _ in range(2)]
        stats, dn, dp = runs[0]
        for a, b in zip(*runs):                                           # reruns are bit-identical
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), term
        assert torch.isfinite(stats[:4]).all() and torch.isfinite(dn).all() and torch.isfinite(dp).all()
        others = [j for j in range(3) if j != k]
        assert not stats[others].any()                                    # a term that is not enabled: exactly 0
        r64, r32 = c["r64"][term], c["r32"][term]
        _check(f"{name} {term} loss", stats[k].item(), r64["loss"], r32["loss"])
        _check(f"{name} {term} dnormal", dn.cpu().numpy(), r64["dnormal"], r32["dnormal"])
        if term == "hole":
            _check(f"{name} {term} dposition", dp.cpu().numpy(), r64["dposition"], r32["dposition"])
        else:
            assert not dp.any() and not r64["dposition"].any()           # exactly 0 unless HOLE is set
        # fused: the same loss, and with dloss on this term alone the same gradients
        assert torch.equal(fused_stats[k], stats[k]), term
        again = _raw(g, 7, _one_hot(term))
        assert torch.equal(again[0].view(torch.int32), fused_stats.view(torch.int32))
        assert torch.equal(again[1], dn) and torch.equal(again[2], dp), term
    # all three at once: the gradient of the sum
    total64 = sum(c["r64"][t]["dnormal"] for t in TERMS)
    total32 = sum(c["r32"][t]["dnormal"] for t in TERMS)
    _check(f"{name} fused dnormal", fused_dn.cpu().numpy(), total64, total32)
    assert torch.equal(fused_dp, _raw(g, 4, _one_hot("hole"))[2])
    assert torch.equal(_raw(g, 7)[1].view(torch.int32), fused_dn.view(torch.int32))


def _view(g):
    from garmentdreamer_amd import mesh_losses as ml
    return ml.View(g["T"], g["tmask"], g["R"], g["center"])


def _gbuffers(g, leaf=True):
    own = {k: g[k].clone().requires_grad_(leaf) for k in ("normal", "position", "mask")}
    return own, {k: g[k + "_rf"] for k in ("normal", "position", "mask")}


def test_public_functions_are_the_mean_over_the_views():
    from garmentdreamer_amd import mesh_losses as ml
    names = ["5x7", "67x131"]
    gs = [_gpu_case(n) for n in names]
    views = [_view(g) for g in gs]
    raw = {t: [_raw(g, BIT[t], _one_hot(t, 0.5)) for g in gs] for t in TERMS}
    calls = {"enhanced": lambda own, rf: ml.normal_map_loss_enhanced(views, own),
             "plain": lambda own, rf: ml.normal_map_loss(views, own),
             "hole": lambda own, rf: ml.hole_mask_loss(views, own, rf)}
    for k, term in enumerate(TERMS):
        own, rf = zip(*[_gbuffers(g) for g in gs])
        loss = calls[term](list(own), list(rf))
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
        assert torch.equal(loss.detach(), (raw[term][0][0][k] + raw[term][1][0][k]) / 2)
        loss.backward()
        for i in range(2):
            assert torch.equal(own[i]["normal"].grad, raw[term][i][1]), (term, i)
            assert own[i]["mask"].grad is None
            if term == "hole":
                assert torch.equal(own[i]["position"].grad, raw[term][i][2])
            else:
                assert own[i]["position"].grad is None
    for enhanced in (True, False):
        own, rf = zip(*[_gbuffers(g) for g in gs])
        losses = ml.second_stage_losses(views, list(own), list(rf), enhanced=enhanced)
        assert sorted(losses) == ["hole_mask", "normal", "normal_enhanced", "normal_plain"]
        for key, (k, term) in (("normal_enhanced", (0, "enhanced")), ("normal_plain", (1, "plain")), ("hole_mask", (2, "hole"))):
            assert torch.equal(losses[key].detach(), (raw[term][0][0][k] + raw[term][1][0][k]) / 2), key
        assert losses["normal"] is losses["normal_enhanced" if enhanced else "normal_plain"]
        (losses["normal"] + losses["hole_mask"]).backward()
        fused = [_raw(g, 7, (0.5 if enhanced else 0.0, 0.0 if enhanced else 0.5, 0.5)) for g in gs]
        for i in range(2):
            assert torch.equal(own[i]["normal"].grad, fused[i][1]) and torch.equal(own[i]["position"].grad, fused[i][2])
    with pytest.raises(ValueError, match="resolution"):
        ml.normal_map_loss([views[0]], [_gbuffers(gs[1])[0]])


# ---- hand-built pixels -------------------------------------------------------------------------------------------------------

def _flat(pixels):
    """A 1 x n case from per-pixel dicts over the defaults: R = I, center = (0, 0, 3), everything covered, normals and the
    normal map facing the camera."""
    n = len(pixels)
    base = {"normal": (0.0, 0.0, 1.0), "position": (0.0, 0.0, 0.0), "mask": 1.0, "normal_rf": (0.0, 0.0, 1.0),
            "position_rf": (0.0, 0.0, 0.0), "mask_rf": 1.0, "T": (0.5, 0.5, 0.0), "tmask": 1.0}
    case = {"R": np.eye(3, dtype=np.float32), "center": np.array([0.0, 0.0, 3.0], np.float32)}
    for k, v in base.items():
        rows = np.array([px.get(k, v) for px in pixels], dtype=np.float32)
        case[k] = rows.reshape(1, n, 3 if rows.ndim == 2 else 1)
    return case


def test_a_cosine_of_exactly_zero_is_in_the_enhanced_mask_and_has_hole_sign_plus_one():
    """p = 0, center = (0, 0, 3), R = I: d = (0, 0, 1) exactly; n = (1, 0, 0): cv = 0 exactly.  The normal map (0.5, 0.5, 0)
    is t = (0, 0, -1): ct = -1 <= epsilon.  So the pixel is in (cv <= 0), e = 1 - 0 = 1, w = exp(1), Z = w: the loss is 1.
    The reference pixel has n_rf = (0, 0, 1), n_cam = (0, 0, -1): cv_rf = -1, s_rf = -1; with s = +1 the hole term is 4."""
    case = _flat([{"normal": (1.0, 0.0, 0.0)}])
    stats, dn, dp = _raw({k: _dev(v) for k, v in case.items()}, 7)
    assert stats[0].item() == 1.0 and stats[2].item() == 4.0
    assert abs(stats[3].item() - np.exp(1.0)) <= 1e-6 * np.exp(1.0)
    assert stats[4:].view(torch.int32).tolist() == [1, 1]
    assert torch.isfinite(dn).all() and torch.isfinite(dp).all() and dn.abs().max() > 0 and dp.abs().max() > 0
    for dtype in (torch.float64, torch.float32):                          # the statement says the same
        c = lref.tensors(case, dtype)
        assert float(lref.enhanced(c)) == 1.0 and float(lref.hole(c)) == 4.0


def test_an_uncovered_view_gives_exact_zeros():
    g = dict(_gpu_case("67x131"))
    g["mask"] = torch.zeros_like(g["mask"])
    for terms in (1, 2, 4, 7):
        stats, dn, dp = _raw(g, terms)
        assert not stats[:3].any() and stats[4:].view(torch.int32).tolist() == [0, 0], terms
        assert not dn.any() and not dp.any(), terms
        assert (stats[3].item() > 0) == bool(terms & 1)                   # Z sums over all pixels, covered or not
    from garmentdreamer_amd import mesh_losses as ml
    own, rf = _gbuffers(g)
    losses = ml.second_stage_losses([_view(g)], [own], [rf])
    (losses["normal_enhanced"] + losses["normal_plain"] + losses["hole_mask"]).backward()
    assert not own["normal"].grad.any() and not own["position"].grad.any()
    assert all(v.item() == 0.0 for v in losses.values())


def test_background_pixels_and_a_position_at_the_centre_stay_finite():
    """n = 0 and p = 0 where nothing was rendered (covered or not, as antialiasing leaves them); p == center: v = 0, u = 0,
    d = 0, every cosine with d is 0 / (1e-6 ...) = 0.  One ordinary pixel keeps the sums from being empty."""
    zero = (0.0, 0.0, 0.0)
    case = _flat([{}, {"normal": zero, "mask": 0.0}, {"normal": zero, "mask": 0.3}, {"normal": zero, "normal_rf": zero},
                  {"position": (0.0, 0.0, 3.0)}, {"position": (0.0, 0.0, 3.0), "normal_rf": (0.0, 0.0, -1.0)},
                  {"position_rf": (0.0, 0.0, 3.0), "normal": (0.0, 0.0, -1.0)}, {"T": zero}, {"T": (0.5, 0.5, 0.5)}])
    g = {k: _dev(v) for k, v in case.items()}
    for terms in (1, 2, 4, 7):
        for t in _raw(g, terms):
            assert torch.isfinite(t[:4] if t.dim() == 1 else t).all(), terms
    stats, dn, dp = _raw(g, 7)
    assert stats[4:].view(torch.int32).tolist() == [8, 8]
    for k, term in enumerate(TERMS):                                      # and the values are the statement's
        want = float(lref.LOSSES[term](lref.tensors(case, torch.float64)))
        assert abs(stats[k].item() - want) <= 1e-6 * max(abs(want), 1.0), (term, stats[k].item(), want)


# ---- the deformer's second stage --------------------------------------------------------------------------------------------

RES = (64, 64)
FLIP = np.diag([1.0, -1.0, -1.0])


@functools.lru_cache(maxsize=None)
def _deformer_scene():
    """The scene of tests/test_mesh_geometry_gpu.py: tube(24, 12), two views at 64 x 64 (the second mirrors world x), target
    masks and target normal maps rendered from the tube translated by 0.05.  A view's R takes the world to a camera that
    looks along +z with y down, so that Rf R n is the normal in the OpenGL camera's frame, as the reference has it."""
    from garmentdreamer_amd import mesh_deform as md
    v, tri, vn = scenes.tube()
    pose = scenes.look_at_pose(scenes.CAMPOS).astype(np.float64)
    mvp = scenes.perspective(scenes.FOVY) @ np.linalg.inv(pose)
    mirror = np.diag([-1.0, 1.0, 1.0])
    mvps = [_dev(mvp.astype(np.float32)), _dev((mvp @ np.diag([-1.0, 1, 1, 1])).astype(np.float32))]
    Rs = [FLIP @ pose[:3, :3].T, FLIP @ pose[:3, :3].T @ mirror]
    centers = [pose[:3, 3], mirror @ pose[:3, 3]]
    Rs, centers = [_dev(R.astype(np.float32)) for R in Rs], [_dev(c.astype(np.float32)) for c in centers]
    v_d, tri_d, vn_d = _dev(v.astype(np.float32)), _dev(tri.astype(np.int32)), _dev(vn.astype(np.float32))
    moved = v_d + torch.tensor([0.05, 0.0, 0.0], device=DEV)
    with torch.no_grad():
        rendered = md.GBufferRenderer().render(mvps, moved, tri_d, vn_d, RES, ["mask", "normal"])
    masks = [r["mask"] for r in rendered]
    normals = [(0.5 * (lref.to_camera(r["normal"], R) + 1)).contiguous() for r, R in zip(rendered, Rs)]
    return v_d, tri_d, mvps, masks, normals, Rs, centers


def _second_stage(first_steps=3, **kw):
    from garmentdreamer_amd.deformer import Deformer
    v, tri, mvps, masks, normals, Rs, centers = _deformer_scene()
    d = Deformer(v, tri, mvps, masks, RES)
    for _ in range(first_steps):
        d.step([0, 1])
    d.begin_second_stage(normals, Rs, centers, **kw)
    return d


def _composition_gradient(d, offsets, dtype):
    """``offsets.grad`` of the second-stage total at ``offsets`` with the two G-buffer losses written as the torch
    composition of tests/mesh_losses_reference.py in ``dtype`` on the SAME render (the package's kernels, float32)."""
    from garmentdreamer_amd import mesh_geometry as mg
    from garmentdreamer_amd.deformer import CHANNELS
    leaf = offsets.clone().requires_grad_(True)
    vertices = d.initial + leaf
    fn, vn = mg.normals(vertices, d.geometry)
    views = [0, 1]
    res = [d.resolutions[i] for i in views]
    gb = d.renderer.render(d.mvps, vertices, d.geometry.tri, vn, res, CHANNELS, with_antialiasing=True,
                           topology=d.geometry.topology)
    with torch.no_grad():
        rf = d.renderer.render(d.mvps, d.rf_vertices, d.rf_geometry.tri, d.rf_normals, res, CHANNELS,
                               with_antialiasing=True, topology=d.rf_geometry.topology)
    normal = hole = 0.0
    for i in views:
        c = {"normal": gb[i]["normal"], "position": gb[i]["position"], "mask": gb[i]["mask"], "normal_rf": rf[i]["normal"],
             "position_rf": rf[i]["position"], "mask_rf": rf[i]["mask"], "T": d.views[i].normal, "tmask": d.views[i].mask,
             "R": d.views[i].R, "center": d.views[i].center}
        c = {k: t.to(dtype) for k, t in c.items()}
        normal = normal + lref.enhanced(c) / 2
        hole = hole + lref.hole(c) / 2
    w = d.second_weights
    total = (w["mask"] * mg.mask_loss([d.target_masks[i] for i in views], gb)
             + w["normal_consistency"] * mg.normal_consistency_loss(fn, d.geometry)
             + w["laplacian"] * mg.laplacian_loss(vertices, d.geometry)).to(dtype) + w["normal"] * normal + w["hole_mask"] * hole
    total.backward()
    return leaf.grad.cpu().numpy(), {"normal": float(normal.detach()), "hole_mask": float(hole.detach())}


def _step_and_compositions(d):
    before = d.offsets.detach().clone()
    out = d.step_second([0, 1])
    got = d.offsets.grad.cpu().numpy()
    g64, l64 = _composition_gradient(d, before, torch.float64)
    g32, _ = _composition_gradient(d, before, torch.float32)
    print("normal", out["normal"].item(), l64["normal"], "hole_mask", out["hole_mask"].item(), l64["hole_mask"])
    return before, out, got, g64, g32


def test_step_second_gradient_against_the_torch_composition_on_the_same_render():
    """``offsets.grad`` after ONE step_second, by the 4x rule.  At that step the mesh still is the frozen reference mesh,
    so the hole-mask term is exactly 0 here; the next test moves away from it."""
    d = _second_stage()
    before, out, got, g64, g32 = _step_and_compositions(d)
    assert sorted(out) == ["hole_mask", "laplacian", "mask", "normal", "normal_consistency", "total"]
    assert all(not t.requires_grad and t.is_cuda and t.dim() == 0 for t in out.values())
    assert out["normal"].item() > 0 and out["hole_mask"].item() == 0.0
    _check("step_second offsets.grad", got, g64, g32)
    # the update: rows outside vertex_visibility are bit-unchanged, the others moved by lr g / (|g| + eps)
    visible = d.renderer.vertex_visibility(d.mvps, d.initial + before, d.geometry.tri, [RES, RES])
    after = d.offsets.detach()
    assert 0 < int(visible.sum()) < visible.shape[0]
    assert torch.equal(after[~visible].view(torch.int32), before[~visible].view(torch.int32))
    g = d.offsets.grad
    assert torch.equal(after[visible], (before - d.lr * g / (g.abs() + 1e-8))[visible])
    assert not torch.equal(after[visible], before[visible])


def test_step_second_gradient_once_the_mesh_has_left_the_reference_mesh():
    """The third step_second: a few pixels now face the other way than the frozen mesh, the hole-mask term is not 0 and
    its gradient reaches the offsets through ``normal`` AND ``position``; with weight 2 over a handful of pixels it
    holds the largest entries of ``offsets.grad``.  The float64 composition hands its G-buffer gradients to the float32
    backward of the render, so ``g64`` is itself rounded to float32 and known only to 2^-24 of its largest entry; the
    float32 composition of those few pixels can agree with it to the bit, which says nothing about a kernel.  Hence the
    4x rule with that resolution as the floor of the reference's error."""
    d = _second_stage()
    for _ in range(2):
        d.step_second([0, 1])
    _, out, got, g64, g32 = _step_and_compositions(d)
    assert out["hole_mask"].item() > 0
    _check("third step_second offsets.grad", got, g64, g32, floor=2.0 ** -24)


def test_step_second_is_reproducible_and_reports_its_losses():
    runs = []
    for _ in range(2):
        d = _second_stage()
        losses = [d.step_second([0, 1]) for _ in range(10)]
        runs.append((d.offsets.detach().clone(), losses))
    assert torch.isfinite(runs[0][0]).all()
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    for a, b in zip(runs[0][1], runs[1][1]):
        assert all(torch.equal(a[k], b[k]) for k in a)
    d = _second_stage()
    losses = [d.step_second([0, 1]) for _ in range(30)]       # printed, not asserted: 30 sign-steps need not descend
    for k in sorted(losses[0]):
        print(f"{k}: step 1 {losses[0][k].item():.6e}, step 30 {losses[-1][k].item():.6e}")
    d = _second_stage(enhanced=False, weights={"normal": 1.0})   # the plain loss alone
    out = d.step_second([1])
    assert out["normal"].item() > 0 and torch.equal(out["total"], out["normal"] * 1.0)
    assert d.offsets.grad.abs().max() > 0


def test_extra_loss_is_added_and_its_gradient_reaches_the_offsets():
    seen = {}

    def extra(view_indices, gbuffers):
        seen["views"], seen["keys"] = list(view_indices), sorted(gbuffers[0])
        return 3.0 * sum((g["position"] ** 2).mean() for g in gbuffers)

    a, b = _second_stage(), _second_stage()
    plain, with_extra = a.step_second([0, 1]), b.step_second([0, 1], extra_loss=extra)
    assert seen == {"views": [0, 1], "keys": ["mask", "normal", "position"]}
    assert with_extra["extra"].item() > 0 and not with_extra["extra"].requires_grad
    assert torch.equal(with_extra["total"], plain["total"] + with_extra["extra"])
    assert all(torch.equal(plain[k], with_extra[k]) for k in plain if k != "total")
    assert not torch.equal(a.offsets.grad, b.offsets.grad)


def test_adopt_remesh():
    from garmentdreamer_amd import mesh_geometry as mg
    d = _second_stage()
    d.step_second([0, 1])
    lr, weights = d.lr, dict(d.second_weights)
    rf_vertices, rf_geometry = d.rf_vertices.clone(), d.rf_geometry
    assert weights == {"hole_mask": 2.0, "mask": 2.0, "normal_consistency": 0.1, "laplacian": 40.0, "normal": 0.8}
    v, tri, _ = scenes.tube(32, 16)                                     # stands for the remeshed surface
    d.adopt_remesh(_dev(v), _dev(tri))
    assert d.lr == lr * 0.25 and d.eps == 1e-8
    want = dict(weights, laplacian=weights["laplacian"] * 4, normal_consistency=weights["normal_consistency"] * 4)
    assert d.second_weights == want
    assert tuple(d.offsets.shape) == tuple(v.shape) and not d.offsets.any() and d.offsets.requires_grad
    assert torch.equal(d.initial, _dev(v)) and d.geometry.num_vertices == v.shape[0]
    assert d.rf_geometry is rf_geometry and torch.equal(d.rf_vertices, rf_vertices)      # the frozen mesh keeps its own
    out = d.step_second([0, 1])
    assert torch.isfinite(out["total"]).item() and d.offsets.detach().abs().max() > 0
    fresh = mg.build_geometry(_dev(tri), num_vertices=v.shape[0], device=DEV)
    assert torch.equal(d.geometry.face_nbr, fresh.face_nbr)


def test_step_second_does_not_synchronise():
    d = _second_stage()
    for _ in range(2):
        d.step_second([0, 1])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = d.step_second([0, 1])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(out["total"]).item()
    from garmentdreamer_amd.deformer import Deformer
    v, tri, mvps, masks, *_ = _deformer_scene()
    with pytest.raises(RuntimeError, match="begin_second_stage"):
        Deformer(v, tri, mvps, masks, RES).step_second([0])
