"""GPU checks of the texture fit (garmentdreamer_amd/texture_fit.py, the entries of include/gd_fit.h in
csrc/raster_fit.hip) against the two statements of tests/fit_reference.py and against ``NeTFRenderer.render``.

Bounds.  With D the longest chain of additions a term of the sum passes through in the header's order
(``fit_reference.chain_length``, from the header's constants) and every term non-negative,
``|loss - loss64| <= (D + 8) 2^-24 loss64``; ``|dc_aa - dc64| <= 16 * 2^-24 * 2 |dloss| / (3 count)`` per element (three
roundings in ``image``, one in the difference, the scale's own); ``image``, ``cosinesview``, ``m`` and ``count`` equal the
float32 statement bit for bit; ``m`` may differ from the float64 mask only where the float64 ``|cos| < 2^-20``, which the
seeding keeps under 0.1 % of the candidates (asserted on the float64 statement alone, here and in the CPU tests).  Through
the render the field's flat gradient is held, by relative L2 distance to the float64 composition on the same render, to four
times the larger distance of the float32 composition in two summation orders (the gather with ``MSELoss``; the masked sum).
Every figure is printed; the measured ones are in DESIGN.md section 3.27."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import fit_reference as fref
from tests import mesh_scenes as scenes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DLOSS = 0.7


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case of a shape and what the CPU says about it in both orientations; computed once, read-only."""
    H, W, seed = fref.SHAPES[name]
    case = fref.make_case(H, W, seed)
    out = {"case": case, "gpu": {k: _dev(v) for k, v in case.items()}}
    for flip in (True, False):
        s32 = fref.statement32(case, flip)
        out[flip] = {"s32": s32, "dc32": fref.backward32(case, s32, DLOSS), "s64": fref.statement64(case, flip, DLOSS)}
    return out


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _raw(g, flip, dloss=DLOSS):
    """Both entries called directly, every output and the scratch pre-filled: (stats [4], image, cosinesview, m, dc_aa)."""
    from garmentdreamer_amd import _native
    L = _native.lib()
    s = torch.cuda.current_stream(DEV).cuda_stream
    H, W = g["a_aa"].shape
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                                   # noqa: E731
    stats, image, cos, dc = _nan(_native.FIT_STATS_WORDS), _nan(H, W, 3), _nan(H, W), _nan(H, W, 3)
    m = torch.full((H, W), 255, dtype=torch.uint8, device=DEV)
    scratch = _nan(L.gd_fit_loss_scratch_bytes(H * W) // 4)
    assert L.gd_fit_loss_forward(s, H, W, int(flip), *[p(g[k]) for k in fref.KEYS], p(image), p(cos), p(m), p(stats),
                                 p(scratch)) == 0
    d = torch.tensor([dloss], dtype=torch.float32, device=DEV)
    assert L.gd_fit_loss_backward(s, H, W, int(flip), p(g["c_aa"]), p(g["a_aa"]), p(g["rgb"]), p(g["bg"]), p(m), p(stats),
                                  p(d), p(dc)) == 0
    return stats, image, cos, m, dc


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("flip", (True, False))
@pytest.mark.parametrize("name", list(fref.SHAPES))
def test_synthetic_buffers_against_both_statements(name, flip):
    c = _case(name)
    s32, dc32, s64 = c[flip]["s32"], c[flip]["dc32"], c[flip]["s64"]
    H, W, _ = fref.SHAPES[name]
    stats, image, cos, m, dc = (t.cpu().numpy() for t in _raw(c["gpu"], flip))
    loss, count, total = float(stats[0]), int(stats.view(np.int32)[1]), stats[2]
    # the float32 statement: bit for bit
    assert np.array_equal(m, s32["m"]) and count == s32["count"]
    assert np.array_equal(_bits(image), _bits(s32["image"]))
    assert np.array_equal(_bits(cos), _bits(s32["cosinesview"]))
    print(f"{name} flip={flip}: sum bit-equal to the float32 statement: {_bits(total) == _bits(s32['sum'])}, "
          f"loss: {_bits(stats[0]) == _bits(s32['loss'])}, dc_aa: {np.array_equal(_bits(dc), _bits(dc32))}")
    # the float64 statement
    candidates, near = int(s64["candidates"].sum()), int(s64["near"].sum())
    assert near < 1e-3 * candidates
    differs = (m != 0) != s64["m"]
    assert not differs[~s64["near"]].any()
    count64 = int(s64["m"].sum())
    assert count64 > 0
    D = fref.chain_length(H * W)
    bound = (D + 8) * fref.U * s64["loss"]
    print(f"  loss {loss:.9g}, float64 {s64['loss']:.17g}, |difference| {abs(loss - s64['loss']):.3e}, D = {D}, allowed "
          f"{bound:.3e}; count {count} ({count64}), {int(differs.sum())} pixels selected differently")
    assert abs(loss - s64["loss"]) <= bound
    allowed = 16 * fref.U * 2 * DLOSS / (3 * count64)
    e = np.abs(dc - s64["dc_aa"])[~differs].max()
    print(f"  dc_aa: max |difference| {e:.3e}, allowed {allowed:.3e}")
    assert np.isfinite(dc).all() and e <= allowed
    assert not dc[m == 0].any()


def test_fit_loss_is_the_entries_and_reruns_are_bit_identical():
    from garmentdreamer_amd import texture_fit as fit
    g = _case("67x131")["gpu"]
    runs = [_raw(g, True), _raw(g, True)]
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    stats, image, cos, m, dc = runs[0]
    c_aa = g["c_aa"].clone().requires_grad_(True)
    buffers = fit.FitBuffers(c_aa, g["a_aa"][..., None], g["p_aa"], g["n_aa"], g["center"])     # alpha as render has it
    loss, image2, cos2, m2 = fit.fit_loss(buffers, g["rgb"], g["tmask"][..., None], bg_color=g["bg"], outputs=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
    assert not image2.requires_grad and m2.dtype == torch.uint8
    assert torch.equal(loss.detach(), stats[0]) and torch.equal(image2, image) and torch.equal(cos2, cos)
    assert torch.equal(m2, m)
    (loss * DLOSS).backward()
    assert torch.equal(c_aa.grad, dc)
    plain = fit.fit_loss(buffers, g["rgb"], g["tmask"], bg_color=[float(x) for x in g["bg"].tolist()], flip_rows=False)
    assert torch.equal(plain.detach(), _raw(g, False)[0][0])
    white = fit.fit_loss(buffers, g["rgb"], g["tmask"])                                        # bg_color = 1
    g1 = dict(g, bg=torch.ones(3, device=DEV))
    assert torch.equal(white.detach(), _raw(g1, True)[0][0])


# ---- through the render ----------------------------------------------------------------------------------------------------------

def _tube_renderer(deterministic=True, grid_seed=1):
    """NeTFRenderer of tube(24, 12) with a small field whose grid has been scaled to +-0.1, its optimizer, pose and proj"""
    from garmentdreamer_amd import mesh_render as mr
    from garmentdreamer_amd import texture_field as tf
    torch.manual_seed(0)
    fld = tf.TextureField(tf.HashGridEncoder.from_layout(tf.grid_layout(16, 2, 1.3, 10),
                                                         generator=torch.Generator().manual_seed(grid_seed)),
                          deterministic=deterministic).to(DEV)
    with torch.no_grad():
        fld.encoder.params.mul_(1e3)
    v, tri, vn = scenes.tube(24, 12)
    netf = tf.NeTFRenderer(_dev(v), _dev(tri), _dev(vn), fld)
    return netf, fld, fld.optimizer(), scenes.look_at_pose(scenes.CAMPOS), mr.perspective(scenes.FOVY)


def _targets(h, w, seed=5):
    rng = np.random.RandomState(seed)
    rgb = rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    tmask = (rng.uniform(0.05, 1, (h, w, 1)) * (rng.uniform(size=(h, w, 1)) >= 0.2)).astype(np.float32)
    return _dev(rgb), _dev(tmask)


def _relative_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("h,w", ((64, 64), (67, 131)))
def test_through_the_render(h, w):
    from garmentdreamer_amd import texture_fit as fit
    netf, fld, opt, pose, proj = _tube_renderer()
    rgb, tmask = _targets(h, w)
    opt.zero_grad()
    loss, image, cos, m = fit.fit_loss(fit.fit_buffers(netf, pose, proj, h, w), rgb, tmask, outputs=True)
    loss.backward()
    got = opt._grad.clone()
    assert torch.isfinite(got).all() and got.abs().max() > 0

    rgb_t, tmask_t = torch.flipud(rgb), torch.flipud(tmask[..., 0])

    def composition(dtype, gather):
        opt.zero_grad()
        out = netf.render(pose, proj, h, w)
        mask = (out["alpha"][..., 0] > 0) & (tmask_t > 0) & (out["cosinesview"] <= 0)
        img, tgt = out["image"].to(dtype), rgb_t.to(dtype)
        if gather:
            value = torch.nn.MSELoss()(img[mask], tgt[mask])
        else:
            value = (((img - tgt) ** 2).sum(-1) * mask).sum() / (3 * mask.sum())
        value.backward()
        return float(value.detach()), opt._grad.clone(), out, mask

    loss64, g64, out, mask = composition(torch.float64, True)
    e_image = float((image - out["image"].detach()).abs().max())
    e_cos = float((cos - out["cosinesview"]).abs().max())
    differs = int(((m != 0) != mask).sum())
    count = int(mask.sum())
    print(f"{h}x{w}: image bit-equal to render(): {torch.equal(image, out['image'])} (max |difference| {e_image:.3e}); "
          f"cosinesview max |difference| {e_cos:.3e}; {count} pixels selected, {differs} selected differently")
    assert e_image <= 2.0 ** -23 and e_cos <= 4 * fref.U and count > 100
    D = fref.chain_length(h * w)
    bound = (D + 8) * fref.U * loss64
    print(f"  loss {loss.item():.9g}, float64 composition {loss64:.17g}, |difference| {abs(loss.item() - loss64):.3e}, "
          f"allowed {bound:.3e}")
    assert abs(loss.item() - loss64) <= bound
    e_f32 = max(_relative_l2(composition(torch.float32, gather)[1], g64) for gather in (True, False))
    e_gpu = _relative_l2(got, g64)
    print(f"  flat gradient: relative L2 distance {e_gpu:.3e}, float32 composition in two orders {e_f32:.3e}, allowed "
          f"{4 * e_f32:.3e}")
    assert e_gpu <= 4 * e_f32
    opt.zero_grad()


def test_an_empty_selection_gives_exact_zeros():
    from garmentdreamer_amd import texture_fit as fit
    netf, fld, opt, pose, proj = _tube_renderer()
    rgb, tmask = _targets(64, 64)
    opt.zero_grad()
    buffers = fit.fit_buffers(netf, pose, proj, 64, 64)
    buffers.c_aa.retain_grad()
    loss, image, cos, m = fit.fit_loss(buffers, rgb, torch.zeros_like(tmask), outputs=True)
    loss.backward()
    assert loss.item() == 0.0 and not m.any() and torch.isfinite(image).all() and torch.isfinite(cos).all()
    assert buffers.c_aa.grad is not None and not buffers.c_aa.grad.any()
    assert not opt._grad.any() and not torch.isnan(opt._grad).any()
    stats, *_, dc = _raw(dict(_case("67x131")["gpu"], tmask=torch.zeros(67, 131, device=DEV)), True)
    assert stats[0].item() == 0.0 and stats.view(torch.int32)[1].item() == 0 and stats[2].item() == 0.0 and not dc.any()


def test_forward_and_backward_twice_are_bit_identical():
    from garmentdreamer_amd import texture_fit as fit
    netf, fld, opt, pose, proj = _tube_renderer(deterministic=True)
    rgb, tmask = _targets(67, 131)
    runs = []
    for _ in range(2):
        opt.zero_grad()
        out = fit.fit_loss(fit.fit_buffers(netf, pose, proj, 67, 131), rgb, tmask, outputs=True)
        out[0].backward()
        runs.append([t.detach().clone() for t in out] + [opt._grad.clone()])
    assert runs[0][-1].abs().max() > 0
    for a, b in zip(*runs):
        assert torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))
    opt.zero_grad()


def test_an_iteration_does_not_synchronise():
    from garmentdreamer_amd import texture_fit as fit
    netf, fld, opt, pose, proj = _tube_renderer()
    rgb, tmask = _targets(64, 64)

    def iteration():
        loss = fit.fit_loss(fit.fit_buffers(netf, pose, proj, 64, 64), rgb, tmask)
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss.detach()

    first = iteration()                       # loads the library and warms the allocators
    before = fld.encoder.params.detach().clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = iteration()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(first) and torch.isfinite(second) and first.item() > 0
    assert not torch.equal(before, fld.encoder.params.detach())


# ---- the loop ----------------------------------------------------------------------------------------------------------------

def _fit_views(res=64):
    """two captured views of a garment of one colour; the permuted positions fit_pose looks from are (1.2, 1.6, 0.9) and
    (-1.4, 1.0, 1.3)"""
    from garmentdreamer_amd import texture_fit as fit
    f = (res / 2) / np.tan(scenes.FOVY / 2)
    K = np.array([[f, 0, res / 2], [0, f, res / 2], [0, 0, 1.0]])
    rgb = torch.tensor([0.2, 0.6, 0.4], device=DEV).expand(res, res, 3).contiguous()
    mask = torch.ones(res, res, 1, device=DEV)
    views = []
    for t in ((0.9, 1.2, 1.6), (1.3, -1.4, 1.0)):
        c2w = np.eye(4)
        c2w[:3, 3] = t
        views.append(fit.FitView(c2w, K, rgb, mask))
    return views


def test_fit_texture_from_mesh_descends_without_synchronising_and_reproducibly():
    views = _fit_views()
    histories = []
    for _ in range(2):
        netf, fld, opt, _, _ = _tube_renderer(deterministic=True)
        netf.fit_texture_from_mesh(views, iters=1, resolution=64, seed=3, optimizer=opt)      # warms the allocators
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            history = netf.fit_texture_from_mesh(views, iters=40, resolution=64, seed=3, optimizer=opt)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert isinstance(history, torch.Tensor) and history.is_cuda and tuple(history.shape) == (40,)
        assert history.dtype == torch.float32 and not history.requires_grad
        histories.append(history)
    h = histories[0].cpu().numpy()
    print("fit: loss at iteration 1", h[0], "at 10", h[9], "at 20", h[19], "at 40", h[-1])
    assert np.isfinite(h).all() and h[0] > 0 and h[-1] < 0.5 * h[0]
    assert torch.equal(histories[0].view(torch.int32), histories[1].view(torch.int32))


def test_fit_texture_from_mesh_builds_its_optimizer_and_refuses_what_it_cannot_fit():
    from garmentdreamer_amd import texture_field as tf
    views = _fit_views(32)
    netf, fld, _, _, _ = _tube_renderer()
    netf2 = tf.NeTFRenderer(netf.v, netf.f, netf.vn, tf.TextureField(
        tf.HashGridEncoder.from_layout(tf.grid_layout(16, 2, 1.3, 10), generator=torch.Generator().manual_seed(1))).to(DEV))
    before = netf2.texture_fn.encoder.params.detach().clone()
    history = netf2.fit_texture_from_mesh(views, iters=2, resolution=32)
    assert tuple(history.shape) == (2,) and torch.isfinite(history).all()
    assert not torch.equal(before, netf2.texture_fn.encoder.params.detach())
    with pytest.raises(TypeError, match="TextureField"):
        tf.NeTFRenderer(netf.v, netf.f, netf.vn, lambda x, mask: x).fit_texture_from_mesh(views, iters=1, resolution=32)
    with pytest.raises(ValueError, match="resolution"):
        netf2.fit_texture_from_mesh(views, iters=1, resolution=48)


# ---- errors --------------------------------------------------------------------------------------------------------------------

def test_errors():
    from garmentdreamer_amd import texture_fit as fit
    g = _case("5x7")["gpu"]
    buffers = fit.FitBuffers(g["c_aa"], g["a_aa"], g["p_aa"], g["n_aa"], g["center"])
    with pytest.raises(ValueError, match="resolution"):
        fit.fit_loss(buffers, torch.zeros(7, 5, 3, device=DEV), g["tmask"])
    with pytest.raises(ValueError, match="resolution"):
        fit.fit_loss(buffers, g["rgb"], torch.zeros(5, 8, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit.fit_loss(buffers, g["rgb"].cpu(), g["tmask"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit.fit_loss(buffers._replace(p_aa=g["p_aa"].cpu()), g["rgb"], g["tmask"])
    for key in ("a_aa", "p_aa", "n_aa", "center"):
        with pytest.raises(NotImplementedError, match="no gradient to " + key):
            fit.fit_loss(buffers._replace(**{key: g[key].clone().requires_grad_(True)}), g["rgb"], g["tmask"])
    with pytest.raises(NotImplementedError, match="no gradient to rgb"):
        fit.fit_loss(buffers, g["rgb"].clone().requires_grad_(True), g["tmask"])
    with pytest.raises(TypeError):
        fit.fit_loss(buffers, g["rgb"].double(), g["tmask"])
    with pytest.raises(ValueError, match=r"\[H,W,3\]"):
        fit.fit_loss(buffers, g["rgb"][..., :2], g["tmask"])
    # an image off a 16-byte boundary is copied, not refused
    shifted = torch.zeros(5 * 7 * 3 + 1, device=DEV)[1:].view(5, 7, 3).copy_(g["rgb"])
    assert shifted.data_ptr() % 16 != 0
    assert torch.equal(fit.fit_loss(buffers, shifted, g["tmask"]), fit.fit_loss(buffers, g["rgb"], g["tmask"]))
