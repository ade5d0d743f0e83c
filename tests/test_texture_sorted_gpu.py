"""GPU checks of the sorted grid gradient (include/gd_texture_sorted.h, csrc/raster_texture_sorted.hip,
``deterministic=True`` of garmentdreamer_amd/texture_field.py) against the float32 statement of its definition
(tests/texture_sorted_reference.py).  ``dgrid`` is compared BIT FOR BIT, the sign of a zero included, on every element.

Sizes: those of tests/test_texture_field_gpu.py, and N = 549: the sort ranks tiles of SORT_TILE = 2 048 items (256 threads
x 8 keys, ``kSortedTile``) and a level has 8 N items, so 549 points are 4 392 items: two full tiles and 296 items of a
third.  Layouts: that file's two, and L = 4, N0 = 1, b = 2, log2_T = 8, whose level 0 has res = 1: corners 1, 2, 4 of
every point share an entry and corners 3, 5, 6 another, which exercises the order by corner.  The fused problems, their
float64 references and their allowances are test_texture_field_gpu's own (shared, computed once)."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_scenes as scenes
from tests import test_texture_field_gpu as fgpu
from tests import texture_reference as tref
from tests import texture_sorted_reference as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SORT_TILE = 2048
MID_TILE = 2 * SORT_TILE // 8 + 37          # 549 points: 8 N = 4 392 = 2 x 2 048 + 296
SIZES = (1, 63, 64, 65, 257, 3001, MID_TILE)
GRADS = fgpu.GRADS


def _tf():
    from garmentdreamer_amd import texture_field as tf
    return tf


def _lib():
    from garmentdreamer_amd import _native
    return _native.lib()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _layout(kw):
    return _tf().grid_layout(kw["num_levels"], kw["base_resolution"], kw["per_level_scale"], kw["log2_hashmap_size"])


def _sort_scratch(n, struct):
    """NaN-filled scratch of exactly the size the query states"""
    return torch.full((max(_lib().gd_texture_sorted_scratch_bytes(n, struct) // 4, 1),), float("nan"), device=DEV)


def _raw_encode_backward_sorted(x, mask, denc, layout, base):
    """gd_texture_encode_backward_sorted adding into a copy of ``base``"""
    n = x.shape[0]
    xg, dg, out = x.to(DEV), denc.to(DEV), base.to(DEV).clone()
    mg = None if mask is None else mask.to(DEV)
    s = layout.struct()
    scratch = _sort_scratch(n, s)
    ret = _lib().gd_texture_encode_backward_sorted(_stream(), n, xg.data_ptr(), None if mg is None else mg.data_ptr(),
                                                   dg.data_ptr(), s, out.data_ptr(), scratch.data_ptr())
    assert ret == 0, _lib().gd_texture_last_error()
    return out


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(sref.LAYOUTS))
def test_encode_backward_sorted_bit_equal(name, n):
    tf = _tf()
    assert MID_TILE * 8 > 2 * SORT_TILE and MID_TILE * 8 % SORT_TILE != 0
    lay, x, mask, denc, base = sref.problem(name, n)
    layout = _layout(sref.LAYOUTS[name])
    want = sref.encode_backward_sorted(x, denc, lay, mask, base)
    got = _raw_encode_backward_sorted(x, mask, denc, layout, base)
    assert sref.bits_equal(got, want), (name, n)                         # every element
    untouched = ~sref.touched(x, lay, mask)
    assert sref.bits_equal(got.cpu()[untouched], base[untouched])         # entries without an item keep their bits
    assert sref.bits_equal(_raw_encode_backward_sorted(x, mask, denc, layout, base), got)       # and again
    # no mask: every point counts
    assert sref.bits_equal(_raw_encode_backward_sorted(x, None, denc, layout, base),
                           sref.encode_backward_sorted(x, denc, lay, None, base))
    # the Python op is the same call: into a zeroed gradient, and into a sink
    grid = torch.zeros(layout.num_params, device=DEV, requires_grad=True)
    tf.encode(x.to(DEV), grid, layout, mask.to(DEV), deterministic=True).backward(denc.to(DEV))
    assert sref.bits_equal(grid.grad, sref.encode_backward_sorted(x, denc, lay, mask))
    enc = tf.HashGridEncoder.from_layout(layout, deterministic=True).to(DEV)
    enc.params._gd_grad_sink = base.to(DEV).clone()
    enc(x.to(DEV), mask=mask.to(DEV)).backward(denc.to(DEV))
    assert sref.bits_equal(enc.params._gd_grad_sink, want)


def test_4096_copies_of_one_point():
    """every entry of the point's cells gets 4 096 items (8 192 where two corners share it): the reference's sequential sum"""
    n = 4096
    for name in ("fused16", "res1"):
        lay = tref.layout(**sref.LAYOUTS[name])
        x = torch.tensor([[0.3, -0.2, 0.7]]).repeat(n, 1)
        denc = torch.from_numpy(np.random.RandomState(4).uniform(-1, 1, size=(n, lay["num_levels"] * 2)).astype(np.float32))
        base = sref.prefilled(int(lay["offset"][-1]) * 2, seed=1)
        got = _raw_encode_backward_sorted(x, None, denc, _layout(sref.LAYOUTS[name]), base)
        assert sref.bits_equal(got, sref.encode_backward_sorted(x, denc, lay, None, base)), name
        assert int((got.cpu().view(torch.int32) != base.view(torch.int32)).sum()) <= lay["num_levels"] * 8 * 2


def test_production_layout_bit_equal():
    n = 4096
    lay, layout = tref.layout(), _tf().grid_layout()
    x = tref.sample_points(n, seed=9)
    denc = torch.from_numpy(np.random.RandomState(9).uniform(-1, 1, size=(n, 32)).astype(np.float32))
    base = sref.prefilled(int(lay["offset"][-1]) * 2, seed=2)
    got = _raw_encode_backward_sorted(x, sref.mask_of(n), denc, layout, base)
    assert sref.bits_equal(got, sref.encode_backward_sorted(x, denc, lay, sref.mask_of(n), base))


def _denc_reference(q, dtype):
    """denc = W1^T dh [N,32] from the header's formulas in ``dtype``; zero rows for the points that take no part"""
    p = {k: v.to(dtype) for k, v in q["p"].items()}
    x, mask = q["x"], q["mask"]
    ok = tref.valid_rows(x.to(dtype), mask)
    enc = tref.encode(x, p["grid"], q["lay"], mask)
    h = torch.relu(enc @ p["w1"].T + p["b1"])
    color = torch.where(ok[:, None], torch.sigmoid(h @ p["w2"].T + p["b2"]), torch.zeros(x.shape[0], 3, dtype=dtype))
    do = (q["dcolor"].to(dtype) * color) * (1 - color)
    dh = (do @ p["w2"]) * (h > 0)
    return torch.where(ok[:, None], dh @ p["w1"], torch.zeros(x.shape[0], 32, dtype=dtype))


def _raw_backward_sorted(q, color, bufs=None, mask="own"):
    """gd_texture_field_backward_sorted adding into ``bufs`` (zeros if not given); returns (bufs, denc)"""
    n = q["xg"].shape[0]
    g = q["gpu"]
    if bufs is None:
        bufs = {"d" + k: torch.zeros_like(v) for k, v in g.items()}
    m = q["maskg"] if isinstance(mask, str) else mask
    L = _lib()
    s = q["layout"].struct()
    slab = torch.full((max(L.gd_texture_field_backward_scratch_bytes(n) // 4, 1),), float("nan"), device=DEV)
    sort = _sort_scratch(n, s)
    denc = torch.full((n, 32), float("nan"), device=DEV)
    ret = L.gd_texture_field_backward_sorted(_stream(), n, q["xg"].data_ptr(), None if m is None else m.data_ptr(),
                                             g["grid"].data_ptr(), s, g["w1"].data_ptr(), g["b1"].data_ptr(),
                                             g["w2"].data_ptr(), g["b2"].data_ptr(), color.data_ptr(),
                                             q["dcolorg"].data_ptr(), *[bufs[k].data_ptr() for k in GRADS],
                                             denc.data_ptr(), slab.data_ptr(), sort.data_ptr())
    assert ret == 0, L.gd_texture_last_error()
    return bufs, denc


@pytest.mark.parametrize("n", SIZES)
def test_field_backward_sorted(n):
    q = fgpu._fused_problem(n)
    color = fgpu._raw_forward(q)
    base = {"d" + k: sref.prefilled(v.numel(), seed=n + i).reshape(v.shape).to(DEV)
            for i, (k, v) in enumerate(q["gpu"].items())}
    got, denc = _raw_backward_sorted(q, color, {k: v.clone() for k, v in base.items()})
    # denc: every element written; against float64 within four times the float32 reference's own error
    assert torch.isfinite(denc).all()
    assert not denc.cpu()[fgpu._dead_rows(q["x"], q["mask"])].any()
    want64 = _denc_reference(q, torch.float64)
    ref32 = fgpu._rel(_denc_reference(q, torch.float32), want64)
    err = fgpu._rel(denc, want64)
    print(f"denc n={n}: gpu {err:.3g} float32 reference {ref32:.3g} allowed {4 * ref32:.3g}")
    assert err <= 4 * ref32, (err, ref32)
    # dgrid: the definition applied to exactly that denc, bit for bit
    want = sref.encode_backward_sorted(q["x"], denc.cpu(), q["lay"], q["mask"], base["dgrid"].cpu())
    assert sref.bits_equal(got["dgrid"], want)
    # the MLP gradients: those of the atomic entry on the same inputs
    atomic = fgpu._raw_backward(q, color, {k: v.clone() for k, v in base.items()})
    for k in ("dw1", "db1", "dw2", "db2"):
        assert torch.equal(got[k], atomic[k]), k
    err = fgpu._rel(got["dgrid"] - base["dgrid"], q["want"]["dgrid"])
    print(f"dgrid n={n}: sorted {err:.3g} allowed {q['allowed']['dgrid']:.3g}")
    # a rerun gives the same bits
    again, denc2 = _raw_backward_sorted(q, color, {k: v.clone() for k, v in base.items()})
    assert torch.equal(denc, denc2) and all(sref.bits_equal(again[k], got[k]) for k in GRADS)


def test_all_zero_mask_leaves_prefilled_buffers_bit_unchanged():
    q = fgpu._fused_problem(257)
    zeros = torch.zeros(257, dtype=torch.uint8, device=DEV)
    color = fgpu._raw_forward(q, mask=zeros)
    base = {"d" + k: sref.prefilled(v.numel(), seed=3).reshape(v.shape).to(DEV) for k, v in q["gpu"].items()}
    for k in ("dw1", "db1", "dw2", "db2"):
        base[k] = torch.full_like(base[k], 0.25)                          # + 0 leaves 0.25 as it is
    got, denc = _raw_backward_sorted(q, color, {k: v.clone() for k, v in base.items()}, mask=zeros)
    assert not denc.any()
    for k in GRADS:
        assert sref.bits_equal(got[k], base[k]), k                       # dgrid is never touched: its -0.0 stay
    lay, x, _, d8, b8 = sref.problem("enc4", 257)
    out = _raw_encode_backward_sorted(x, torch.zeros(257, dtype=torch.uint8), d8, _layout(sref.LAYOUTS["enc4"]), b8)
    assert sref.bits_equal(out, b8)


def _module(q, deterministic):
    fld = fgpu._module(q)
    fld.encoder.deterministic = deterministic
    return fld


def test_module_routes_on_the_flag():
    """``TextureField.forward``, ``.unfused`` and ``.encoder`` follow ``encoder.deterministic``; the forwards are untouched"""
    tf = _tf()
    q = fgpu._fused_problem(257)
    base = fgpu._module(q)
    assert base.encoder.deterministic is False
    results = []
    for _ in range(2):
        fld = tf.TextureField(tf.HashGridEncoder.from_layout(q["layout"]), deterministic=True).to(DEV)
        assert fld.encoder.deterministic is True
        with torch.no_grad():
            fld.encoder.params.copy_(q["gpu"]["grid"])
            for dst, k in zip(fld.mlp.parameters(), ("w1", "b1", "w2", "b2")):
                dst.copy_(q["gpu"][k])
        color = fld(q["xg"], q["maskg"])
        assert torch.equal(color, base(q["xg"], q["maskg"]))
        (color * q["dcolorg"]).sum().backward()
        fused = fgpu._module_grads(fld)
        _, denc = _raw_backward_sorted(q, color.detach())
        assert sref.bits_equal(fused["dgrid"], sref.encode_backward_sorted(q["x"], denc.cpu(), q["lay"], q["mask"]))
        for k in GRADS:
            assert fgpu._rel(fused[k], q["want"][k]) <= q["allowed"][k], k
        unf = tf.TextureField(tf.HashGridEncoder.from_layout(q["layout"]), deterministic=True).to(DEV)
        with torch.no_grad():
            unf.encoder.params.copy_(q["gpu"]["grid"])
            for dst, k in zip(unf.mlp.parameters(), ("w1", "b1", "w2", "b2")):
                dst.copy_(q["gpu"][k])
        (unf.unfused(q["xg"], q["maskg"]) * q["dcolorg"]).sum().backward()
        assert fgpu._rel(unf.encoder.params.grad, q["want"]["dgrid"]) <= q["allowed"]["dgrid"]
        results.append(fused["dgrid"].clone())
    assert torch.equal(results[0], results[1])


def _fit(deterministic, steps=10):
    """(flat parameter buffer, last loss) of a fit of 0.5 + 0.5 sin(3x) on 2 048 points from fixed seeds"""
    tf = _tf()
    torch.manual_seed(0)
    enc = tf.HashGridEncoder.from_layout(tf.grid_layout(16, 2, 1.3, 10), generator=torch.Generator().manual_seed(1))
    fld = tf.TextureField(enc, deterministic=deterministic).to(DEV)
    opt = fld.optimizer()
    x = torch.from_numpy(np.random.RandomState(2).uniform(-1, 1, size=(2048, 3)).astype(np.float32)).to(DEV)
    target = 0.5 + 0.5 * torch.sin(3 * x)
    loss = None
    for _ in range(steps):
        opt.zero_grad()
        loss = ((fld(x) - target) ** 2).mean()
        loss.backward()
        opt.step()
    return opt._flat.detach().clone(), float(loss.detach())


@functools.lru_cache(maxsize=None)
def _fits():
    return _fit(True), _fit(True), _fit(False)


def test_two_deterministic_fits_are_bit_equal():
    """the user-visible property: same seeds, ten optimizer steps, the same parameters bit for bit"""
    (flat_a, loss_a), (flat_b, loss_b), _ = _fits()
    assert torch.equal(flat_a, flat_b) and loss_a == loss_b
    assert torch.isfinite(flat_a).all()


def test_deterministic_fit_loss_is_the_atomic_fits():
    """A sanity check, no bit-level claim: the loss after ten steps through the sorted path against the loss through the
    atomic path, relative, within the atomic path's allowance: the largest of test_texture_field_gpu's allowances (four
    times the float32 reference's own error against float64) over ``color`` and the five gradients of its fused problem at
    3 001 points, the same layout.  Both paths add the same float32 contributions in another order, so each is within that
    allowance of the float64 gradient; Adam's step ``m / (sqrt(v) + eps)`` does not amplify a relative perturbation of the
    gradient, and ten steps at 1e-2 / 1e-3 move the loss by less than its own size."""
    (_, det), _, (_, atomic) = _fits()
    allowed = max(fgpu._fused_problem(3001)["allowed"].values())
    print(f"fit, loss after 10 steps: sorted {det!r} atomic {atomic!r} relative {abs(det - atomic) / atomic:.3g} "
          f"allowed {allowed:.3g}")
    assert abs(det - atomic) <= allowed * atomic


def test_netf_render_backward_step_with_a_deterministic_field_never_wait_for_the_gpu():
    tf = _tf()
    from garmentdreamer_amd import mesh_render as mr
    q = fgpu._fused_problem(257)
    v, tri, vn = scenes.tube(24, 12)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pose, proj = scenes.look_at_pose(scenes.CAMPOS), mr.perspective(scenes.FOVY)
    fld = _module(q, True)
    opt = fld.optimizer()
    netf = tf.NeTFRenderer(dv(v), dv(tri), dv(vn), fld)
    target = torch.rand(48, 64, 3, device=DEV)

    def iteration():
        opt.zero_grad()
        out = netf.render(pose, proj, 48, 64)
        loss = ((out["image"] - target) ** 2).mean()
        loss.backward()
        opt.step()
        return loss.detach()

    first = iteration()                       # loads the library and warms the allocators
    before = fld.encoder.params.detach().clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = iteration()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(first) and torch.isfinite(second)
    assert not torch.equal(before, fld.encoder.params.detach())      # the step moved the grid
