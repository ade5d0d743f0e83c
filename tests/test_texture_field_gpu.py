"""GPU checks of the texture field (csrc/raster_texture.hip, garmentdreamer_amd/texture_field.py) against the CPU statement
of its definitions (tests/texture_reference.py).

The encoding is compared bit for bit with the float32 reference.  ``color`` and every gradient are measured as
``max|g - g64| / max|g64|`` against the float64 reference (the measure of the mesh gradients), and the allowance is FOUR
times the same error of the float32 reference on the same input; for the sums over points (``dgrid`` and the four MLP
gradients) that is the largest error over three summation orders, the three of the deformer's losses
(mesh_geometry_reference.scalar_sums): torch's own sum (its matrix product, here over shuffled points), the ascending
running sum and the descending running sum, one float32 sum being a sample that can be exact by chance.  Figures measured
on one MI355X are in DESIGN.md 3.20.

Layouts: encoder-only L = 4, N0 = 3, b = 2, log2_T = 8 (a dense level padded 27 -> 32, a dense level, two hashed);
fused L = 16, N0 = 2, b = 1.3, log2_T = 10 (seven dense levels, nine hashed); the production layout once."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_scenes as scenes
from tests import texture_reference as tref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 63, 64, 65, 257, 3001)
ENC_KW = dict(num_levels=4, base_resolution=3, per_level_scale=2.0, log2_hashmap_size=8)
FUSED_KW = dict(num_levels=16, base_resolution=2, per_level_scale=1.3, log2_hashmap_size=10)
GRADS = ("dgrid", "dw1", "db1", "dw2", "db2")


def _tf():
    from garmentdreamer_amd import texture_field as tf
    return tf


def _lib():
    from garmentdreamer_amd import _native
    return _native.lib()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _rel(got, want64):
    return float((got.detach().cpu().double().reshape(want64.shape) - want64).abs().max() / want64.abs().max())


def _orders(n, seed=11):
    """(order of the points, running sums instead of torch's): torch's sum, ascending sequential, descending sequential"""
    return [(torch.from_numpy(np.random.RandomState(seed).permutation(n)), False), (None, True),
            (torch.arange(n).flip(0), True)]


def _params(lay, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape, s=1.0: ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * s).to(dtype)
    return dict(grid=rnd(int(lay["offset"][-1]) * 2), w1=rnd(32, 32, s=0.3), b1=rnd(32, s=0.3), w2=rnd(3, 32, s=0.3),
                b2=rnd(3, s=0.3))


def _mask(n):
    m = torch.ones(n, dtype=torch.uint8)
    m[4::7] = 0
    return m


def _reference(x, p, lay, dcolor, mask):
    """float64 results and, per quantity, the allowance: 4 x the float32 reference's error (largest over three orders)"""
    p64 = {k: v.double() for k, v in p.items()}
    want = tref.field_backward(x, p64["grid"], p64["w1"], p64["b1"], p64["w2"], p64["b2"], lay, dcolor.double(), mask)
    ref32 = {k: 0.0 for k in want}
    untouched = None
    for order, sequential in _orders(x.shape[0]):
        got = tref.field_backward(x, p["grid"], p["w1"], p["b1"], p["w2"], p["b2"], lay, dcolor, mask, order, sequential)
        if untouched is None:
            untouched = got["dgrid"] == 0     # from float32: the GPU forms the same cells bit for bit, float64 need not
        for k in want:
            ref32[k] = max(ref32[k], _rel(got[k], want[k]))
    return want, ref32, {k: 4 * v for k, v in ref32.items()}, untouched


@functools.lru_cache(maxsize=None)
def _fused_problem(n, masked=True):
    """Inputs, float64 reference and allowances of the fused layout at ``n`` points; shared and treated as read-only."""
    lay = tref.layout(**FUSED_KW)
    p = _params(lay, seed=n)
    x = tref.sample_points(n, seed=n)
    mask = _mask(n) if masked else None
    dcolor = torch.from_numpy(np.random.RandomState(n).uniform(-1, 1, size=(n, 3)).astype(np.float32))
    want, ref32, allowed, untouched = _reference(x, p, lay, dcolor, mask)
    gpu = {k: v.to(DEV) for k, v in p.items()}
    return dict(lay=lay, layout=_tf().grid_layout(16, 2, 1.3, 10), p=p, gpu=gpu, x=x, xg=x.to(DEV), mask=mask,
                maskg=None if mask is None else mask.to(DEV), dcolor=dcolor, dcolorg=dcolor.to(DEV), want=want,
                ref32=ref32, allowed=allowed, untouched=untouched)


def _raw_forward(q, color=None, mask="own"):
    """gd_texture_field_forward into ``color`` (NaN-filled if not given)"""
    n = q["xg"].shape[0]
    color = torch.full((n, 3), float("nan"), device=DEV) if color is None else color
    m = q["maskg"] if isinstance(mask, str) else mask
    g = q["gpu"]
    ret = _lib().gd_texture_field_forward(_stream(), n, q["xg"].data_ptr(), None if m is None else m.data_ptr(),
                                          g["grid"].data_ptr(), q["layout"].struct(), g["w1"].data_ptr(),
                                          g["b1"].data_ptr(), g["w2"].data_ptr(), g["b2"].data_ptr(), color.data_ptr())
    assert ret == 0, _lib().gd_texture_last_error()
    return color


def _raw_backward(q, color, bufs=None, mask="own"):
    """gd_texture_field_backward adding into ``bufs`` (zeros if not given); the scratch starts as NaN"""
    n = q["xg"].shape[0]
    g = q["gpu"]
    if bufs is None:
        bufs = {"d" + k: torch.zeros_like(v) for k, v in g.items()}
    m = q["maskg"] if isinstance(mask, str) else mask
    L = _lib()
    scratch = torch.full((max(L.gd_texture_field_backward_scratch_bytes(n) // 4, 1),), float("nan"), device=DEV)
    ret = L.gd_texture_field_backward(_stream(), n, q["xg"].data_ptr(), None if m is None else m.data_ptr(),
                                      g["grid"].data_ptr(), q["layout"].struct(), g["w1"].data_ptr(), g["b1"].data_ptr(),
                                      g["w2"].data_ptr(), g["b2"].data_ptr(), color.data_ptr(), q["dcolorg"].data_ptr(),
                                      *[bufs[k].data_ptr() for k in GRADS], scratch.data_ptr())
    assert ret == 0, L.gd_texture_last_error()
    return bufs


def _dead_rows(x, mask):
    dead = ~torch.isfinite(x).all(dim=1)
    return dead if mask is None else dead | (mask == 0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kw", (ENC_KW, FUSED_KW), ids=("enc4", "fused16"))
def test_encode_forward_bit_equal(kw, n):
    tf = _tf()
    lay = tref.layout(**kw)
    layout = tf.grid_layout(kw["num_levels"], kw["base_resolution"], kw["per_level_scale"], kw["log2_hashmap_size"])
    grid = torch.from_numpy(np.random.RandomState(7).uniform(-1, 1, int(lay["offset"][-1]) * 2).astype(np.float32))
    x, mask = tref.sample_points(n, seed=n + 1), _mask(n)
    want = tref.encode(x, grid, lay, mask)
    enc = torch.full((n, lay["num_levels"] * 2), float("nan"), device=DEV)
    gg, xg, mg = grid.to(DEV), x.to(DEV), mask.to(DEV)
    ret = _lib().gd_texture_encode_forward(_stream(), n, xg.data_ptr(), mg.data_ptr(), gg.data_ptr(), layout.struct(),
                                           enc.data_ptr())
    assert ret == 0
    assert torch.isfinite(enc).all()                                   # every element written
    assert torch.equal(enc.cpu(), want)
    assert not enc.cpu()[_dead_rows(x, mask)].any()                   # exactly 0
    assert torch.equal(tf.encode(xg, gg, layout, mg), enc)             # the Python op is the same call
    assert torch.equal(tf.encode(xg, gg, layout, mg.bool()), enc)
    # mask=None is an all-ones mask
    assert torch.equal(tf.encode(xg, gg, layout).cpu(), tref.encode(x, grid, lay))
    assert torch.equal(tf.encode(xg, gg, layout), tf.encode(xg, gg, layout, torch.ones_like(mg)))


@pytest.mark.parametrize("n", SIZES)
def test_encode_backward(n):
    tf = _tf()
    lay = tref.layout(**ENC_KW)
    layout = tf.grid_layout(4, 3, 2.0, 8)
    x, mask = tref.sample_points(n, seed=n + 2), _mask(n)
    denc = torch.from_numpy(np.random.RandomState(n).uniform(-1, 1, size=(n, 8)).astype(np.float32))
    want = tref.encode_backward(x, denc.double(), lay, mask)
    ref32, untouched = 0.0, None
    for order, _ in _orders(n):
        perm = torch.arange(n) if order is None else order
        got32 = tref.encode_backward(x[perm], denc[perm], lay, mask[perm])
        untouched = got32 == 0 if untouched is None else untouched
        ref32 = max(ref32, _rel(got32, want))
    grid = torch.zeros(int(lay["offset"][-1]) * 2, device=DEV, requires_grad=True)
    enc = tf.encode(x.to(DEV), grid, layout, mask.to(DEV))
    enc.backward(denc.to(DEV))
    err = _rel(grid.grad, want)
    print(f"encode dgrid n={n}: gpu {err:.3g} float32 reference {ref32:.3g} allowed {4 * ref32:.3g}")
    assert torch.isfinite(grid.grad).all() and err <= 4 * ref32
    assert torch.equal(grid.grad.cpu() == 0, untouched)               # the same entries are touched


@pytest.mark.parametrize("n", SIZES)
def test_field_forward_and_gradients(n):
    q = _fused_problem(n)
    color = _raw_forward(q)
    assert torch.isfinite(color).all()
    assert not color.cpu()[_dead_rows(q["x"], q["mask"])].any()
    got = dict(_raw_backward(q, color), color=color)
    for k in ("color",) + GRADS:
        err = _rel(got[k], q["want"][k])
        print(f"{k} n={n}: gpu {err:.3g} float32 reference {q['ref32'][k]:.3g} allowed {q['allowed'][k]:.3g}")
        assert torch.isfinite(got[k]).all() and err <= q["allowed"][k], (k, err, q["allowed"][k])
    assert torch.equal(got["dgrid"].cpu() == 0, q["untouched"])     # nothing written outside the cells of the points


def test_contention_4096_copies_of_one_point():
    lay = tref.layout(**FUSED_KW)
    p = _params(lay, seed=5)
    one = torch.tensor([[0.3, -0.2, 0.7]])
    d1 = torch.tensor([[0.9, -0.4, 0.6]])
    n = 4096
    q = dict(lay=lay, layout=_tf().grid_layout(16, 2, 1.3, 10), p=p, gpu={k: v.to(DEV) for k, v in p.items()},
             x=one.repeat(n, 1), xg=one.repeat(n, 1).to(DEV), mask=None, maskg=None, dcolorg=d1.repeat(n, 1).to(DEV))
    p64 = {k: v.double() for k, v in p.items()}
    single = tref.field_backward(one, p64["grid"], p64["w1"], p64["b1"], p64["w2"], p64["b2"], lay, d1.double())
    want = {k: single[k] * n for k in GRADS}
    many32 = [tref.field_backward(q["x"], p["grid"], p["w1"], p["b1"], p["w2"], p["b2"], lay, d1.repeat(n, 1),
                                  sequential=sequential) for sequential in (False, True)]   # copies: the orders coincide
    got = _raw_backward(q, _raw_forward(q))
    for k in GRADS:
        ref32, err = max(_rel(m[k], want[k]) for m in many32), _rel(got[k], want[k])
        print(f"{k} 4096 copies: gpu {err:.3g} float32 reference {ref32:.3g} allowed {4 * ref32:.3g}")
        assert err <= 4 * ref32, (k, err, ref32)
    assert int((got["dgrid"] != 0).sum()) <= 16 * 8 * 2               # one cell per level


def test_reruns_forward_and_mlp_gradients_bit_identical():
    q = _fused_problem(3001)
    c1, c2 = _raw_forward(q), _raw_forward(q)
    assert torch.equal(c1, c2)
    g1, g2 = _raw_backward(q, c1), _raw_backward(q, c1)
    for k in ("dw1", "db1", "dw2", "db2"):
        assert torch.equal(g1[k], g2[k]), k
    # dgrid: float atomics, the last bits depend on the order of arrival -- not asserted equal, both within the allowance
    assert _rel(g2["dgrid"], q["want"]["dgrid"]) <= q["allowed"]["dgrid"]


def test_backward_adds_to_prefilled_buffers():
    q = _fused_problem(257)
    color = _raw_forward(q)
    zero = _raw_backward(q, color)
    base = {k: torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, tuple(v.shape)).astype(np.float32)).to(DEV)
            for k, v in zero.items()}
    got = _raw_backward(q, color, {k: v.clone() for k, v in base.items()})
    for k in ("dw1", "db1", "dw2", "db2"):
        assert torch.equal(got[k], base[k] + zero[k]), k              # dst = dst + (the fixed-order total): one rounding
    untouched = zero["dgrid"] == 0
    assert untouched.any() and torch.equal(got["dgrid"][untouched], base["dgrid"][untouched])
    assert (got["dgrid"][~untouched] != base["dgrid"][~untouched]).any()
    # one point: an entry that receives exactly one contribution is base + that contribution, one rounding
    q1 = _fused_problem(1)
    c = _raw_forward(q1)
    z1 = _raw_backward(q1, c)["dgrid"]
    b1 = base["dgrid"]
    g1 = _raw_backward(q1, c, {k: v.clone() for k, v in base.items()})["dgrid"]
    u = (q1["x"] + 1) * 0.5                                            # float32, as the kernel forms it
    hits = torch.zeros(int(q1["lay"]["offset"][-1]), dtype=torch.int64)
    for l in range(16):
        for idx, _ in tref._cells(u, q1["lay"], l):
            hits.index_add_(0, int(q1["lay"]["offset"][l]) + idx, torch.ones(1, dtype=torch.int64))
    once, never = (hits == 1).repeat_interleave(2).to(DEV), (hits == 0).repeat_interleave(2).to(DEV)
    assert int(once.sum()) >= 100
    assert torch.equal(g1[once], b1[once] + z1[once])
    assert torch.equal(g1[never], b1[never])


def test_masking():
    q = _fused_problem(257)
    n = 257
    zeros = torch.zeros(n, dtype=torch.uint8, device=DEV)
    color = _raw_forward(q, mask=zeros)
    assert not color.any()                                             # NaN-filled before the call
    base = {"d" + k: torch.full_like(v, 0.25) for k, v in q["gpu"].items()}
    got = _raw_backward(q, color, {k: v.clone() for k, v in base.items()}, mask=zeros)
    for k in GRADS:
        assert torch.equal(got[k], base[k]), k                        # + 0 leaves 0.25 as it is; dgrid is never touched
    ones = torch.ones(n, dtype=torch.uint8, device=DEV)
    c_none, c_ones = _raw_forward(q, mask=None), _raw_forward(q, mask=ones)
    assert torch.equal(c_none, c_ones)
    g_none, g_ones = _raw_backward(q, c_none, mask=None), _raw_backward(q, c_ones, mask=ones)
    for k in ("dw1", "db1", "dw2", "db2"):
        assert torch.equal(g_none[k], g_ones[k]), k
    qn = _fused_problem(257, masked=False)
    assert _rel(g_none["dgrid"], qn["want"]["dgrid"]) <= qn["allowed"]["dgrid"]
    assert _rel(g_ones["dgrid"], qn["want"]["dgrid"]) <= qn["allowed"]["dgrid"]


def _module(q, seed=0):
    """a TextureField on the GPU holding the problem's parameters"""
    tf = _tf()
    fld = tf.TextureField(tf.HashGridEncoder.from_layout(q["layout"])).to(DEV)
    with torch.no_grad():
        fld.encoder.params.copy_(q["gpu"]["grid"])
        for dst, k in zip(fld.mlp.parameters(), ("w1", "b1", "w2", "b2")):
            dst.copy_(q["gpu"][k])
    return fld


def _module_grads(fld):
    return dict(zip(GRADS, [fld.encoder.params.grad] + [p.grad for p in fld.mlp.parameters()]))


@functools.lru_cache(maxsize=None)
def _fused_and_unfused():
    """(problem, fused results, unfused results, the fused module) at 3 001 points; shared and treated as read-only"""
    q = _fused_problem(3001)
    a, b = _module(q), _module(q)
    ca = a(q["xg"], q["maskg"])
    cb = b.unfused(q["xg"], q["maskg"])
    (ca * q["dcolorg"]).sum().backward()
    (cb * q["dcolorg"]).sum().backward()
    return q, dict(_module_grads(a), color=ca.detach()), dict(_module_grads(b), color=cb.detach()), a


@pytest.mark.parametrize("k", ("color",) + GRADS)
def test_fused_equals_unfused(k):
    """|fused - unfused| / max|g64| within the allowance, per quantity.  The unfused path is ``.encoder`` followed by
    ``.mlp`` (torch's GEMMs, the weight gradients summed in blocks of 128 points) and torch's autograd; both sides are
    also held to the allowance against float64 on their own.  Figures: DESIGN.md 3.20."""
    q, fused, unfused, _ = _fused_and_unfused()
    scale = float(q["want"][k].abs().max())
    diff = float((fused[k] - unfused[k]).abs().max()) / scale
    print(f"{k}: |fused - unfused| / max|g64| {diff:.3g}, fused against float64 {_rel(fused[k], q['want'][k]):.3g}, "
          f"unfused against float64 {_rel(unfused[k], q['want'][k]):.3g}, allowed {q['allowed'][k]:.3g}")
    assert _rel(fused[k], q["want"][k]) <= q["allowed"][k]
    assert diff <= q["allowed"][k]


def test_field_refuses_a_gradient_to_the_positions():
    q, _, _, fld = _fused_and_unfused()
    with pytest.raises(NotImplementedError, match="positions"):
        fld(q["xg"].clone().requires_grad_(True))


def test_production_layout_forward_and_dgrid():
    """the only test that allocates the 45.7 MB table"""
    tf = _tf()
    lay, layout = tref.layout(), tf.grid_layout()
    n = 4096
    p = _params(lay, seed=9)
    x = tref.sample_points(n, seed=9)
    dcolor = torch.from_numpy(np.random.RandomState(9).uniform(-1, 1, size=(n, 3)).astype(np.float32))
    gg, xg = p["grid"].to(DEV), x.to(DEV)
    assert torch.equal(tf.encode(xg, gg, layout).cpu(), tref.encode(x, p["grid"], lay))
    p64 = {k: v.double() for k, v in p.items()}
    want = tref.field_backward(x, p64["grid"], p64["w1"], p64["b1"], p64["w2"], p64["b2"], lay, dcolor.double())
    ref32, untouched = {"color": 0.0, "dgrid": 0.0}, None
    for order, sequential in _orders(n):
        r = tref.field_backward(x, p["grid"], p["w1"], p["b1"], p["w2"], p["b2"], lay, dcolor, None, order, sequential)
        untouched = r["dgrid"] == 0 if untouched is None else untouched
        for k in ref32:
            ref32[k] = max(ref32[k], _rel(r[k], want[k]))
    leaves = [v.to(DEV).requires_grad_(True) for v in (p["grid"], p["w1"], p["b1"], p["w2"], p["b2"])]
    color = tf.field(xg, *leaves, layout)
    color.backward(dcolor.to(DEV))
    for k, got in (("color", color), ("dgrid", leaves[0].grad)):
        err = _rel(got, want[k])
        print(f"production {k}: gpu {err:.3g} float32 reference {ref32[k]:.3g} allowed {4 * ref32[k]:.3g}")
        assert err <= 4 * ref32[k], (k, err)
    assert torch.equal(leaves[0].grad.cpu() == 0, untouched)


def test_optimizer_one_step_from_zero_moments():
    q = _fused_problem(257)
    fld = _module(q)
    opt = fld.optimizer(hashgrid_lr=0.01, mlp_lr=0.001)
    params = [fld.encoder.params] + list(fld.mlp.parameters())
    for p, k in zip(params, ("grid", "w1", "b1", "w2", "b2")):
        assert torch.equal(p.detach(), q["gpu"][k])                   # re-seated, same values
        assert p.grad is not None and not p.grad.any() and p.grad.data_ptr() != 0
    assert params[0].data_ptr() == opt._flat.data_ptr() and params[0].grad.data_ptr() == opt._grad.data_ptr()
    (fld(q["xg"], q["maskg"]) * q["dcolorg"]).sum().backward()
    for k, p in zip(GRADS, params):                                    # the backward wrote straight into the flat buffer
        assert _rel(p.grad, q["want"][k]) <= q["allowed"][k], k
    before = [p.detach().clone() for p in params]
    grads = [p.grad.detach().clone() for p in params]
    opt.step()
    eps = 1e-8
    for p0, g, p, lr in zip(before, grads, params, (0.01, 0.001, 0.001, 0.001, 0.001)):
        g64 = g.double()
        want = p0.double() - lr * g64 / (g64.abs() + eps)
        # a dozen fp32 operations at 2^-24 each on the step (2e-6 of it, as in the deformer's check of the same identity),
        # and the rounding of the subtraction from p itself
        tol = 2e-6 * lr + 2.0 ** -24 * p0.double().abs()
        assert bool(((p.detach().double() - want).abs() <= tol).all())
        moved = g != 0
        assert moved.any() and float((p.detach() - p0)[moved].abs().max()) > 0.5 * lr
        assert torch.equal(p.detach()[~moved], p0[~moved])            # untouched entries: bit-unchanged
    assert (grads[0] == 0).any()                                       # the grid does have untouched entries
    opt.zero_grad()
    assert not opt._grad.any() and all(p.grad is not None and not p.grad.any() for p in params)


def test_fit_sine_colours():
    tf = _tf()
    torch.manual_seed(0)
    fld = tf.TextureField(tf.HashGridEncoder.from_layout(tf.grid_layout(16, 2, 1.3, 10),
                                                         generator=torch.Generator().manual_seed(1))).to(DEV)
    opt = fld.optimizer()
    x = torch.from_numpy(np.random.RandomState(2).uniform(-1, 1, size=(2048, 3)).astype(np.float32)).to(DEV)
    target = 0.5 + 0.5 * torch.sin(3 * x)
    losses = []
    for _ in range(100):
        opt.zero_grad()
        loss = ((fld(x) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    first, last = float(losses[0]), float(losses[-1])
    print("fit: loss at step 1", first, "at step 100", last)
    assert last < first


class _Recorder:
    """texture_fn that keeps what it was given and the gradient of what it returned"""

    def __init__(self, fn):
        self.fn = fn

    def __call__(self, x, *mask):
        self.x, self.mask = x.detach(), (mask[0].detach() if mask else None)
        self.out = self.fn(x, *mask)
        self.out.retain_grad()
        return self.out


def test_netf_renderer_equals_mesh_renderer():
    """``image`` (and the other four outputs) bit-equal to ``MeshRenderer`` with the same field, then the gradients against
    the float64 reference of that path.  Both renderers invert the pose with the same device routine; a host inverse is a
    last bit away from it, and with it the barycentrics and the sampled points."""
    tf = _tf()
    from garmentdreamer_amd import mesh_render as mr
    q = _fused_problem(257)
    v, tri, vn = scenes.tube(24, 12)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pose, proj = scenes.look_at_pose(scenes.CAMPOS), mr.perspective(scenes.FOVY)
    h, w = 48, 64
    fa, fb = _module(q), _module(q)
    ra, rb = _Recorder(fa), _Recorder(fb)
    netf = tf.NeTFRenderer(dv(v), dv(tri), dv(vn), ra)
    mesh = mr.MeshRenderer(dv(v), dv(tri), dv(vn), rb)
    out_a, out_b = netf.render(pose, proj, h, w), mesh.render(pose, proj, h, w)
    for k in ("image", "alpha", "depth", "normal", "cosinesview"):
        assert torch.equal(out_a[k], out_b[k]), k
    visible = ra.mask.bool()
    assert 0.1 < float(visible.float().mean()) < 0.9
    assert torch.equal(ra.x[visible], rb.x)
    target = torch.from_numpy(np.random.RandomState(5).uniform(0, 1, size=(h, w, 3)).astype(np.float32)).to(DEV)
    ((out_a["image"] - target) ** 2).sum().backward()
    ((out_b["image"] - target) ** 2).sum().backward()
    assert torch.equal(ra.out.grad[visible], rb.out.grad)
    # the float64 reference of that path: the field at the visible points under the gradient the render handed it
    x, dcolor = rb.x.cpu(), rb.out.grad.cpu()
    want, ref32, allowed, _ = _reference(x, q["p"], q["lay"], dcolor, None)
    ga, gb = _module_grads(fa), _module_grads(fb)
    for k in GRADS:
        ea, eb = _rel(ga[k], want[k]), _rel(gb[k], want[k])
        between = float((ga[k] - gb[k]).abs().max()) / float(want[k].abs().max())
        print(f"{k} ({x.shape[0]} visible): NeTFRenderer {ea:.3g} MeshRenderer {eb:.3g} between them {between:.3g} "
              f"float32 reference {ref32[k]:.3g} allowed {allowed[k]:.3g}")
        assert ea <= allowed[k] and between <= allowed[k], k


def test_netf_render_backward_step_never_wait_for_the_gpu():
    tf = _tf()
    from garmentdreamer_amd import mesh_render as mr
    q = _fused_problem(257)
    v, tri, vn = scenes.tube(24, 12)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    pose, proj = scenes.look_at_pose(scenes.CAMPOS), mr.perspective(scenes.FOVY)
    fld = _module(q)
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


def test_netf_renderer_refuses_a_singular_pose_as_mesh_renderer_does():
    tf = _tf()
    from garmentdreamer_amd import mesh_render as mr
    v, tri, vn = scenes.tube(24, 12)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    proj = mr.perspective(scenes.FOVY)
    flat = lambda x, *mask: torch.full_like(x, 0.5)
    singular = scenes.look_at_pose(scenes.CAMPOS).copy()
    singular[:, 1] = 0          # a zero column: every LU meets an exactly zero pivot
    for renderer in (tf.NeTFRenderer(dv(v), dv(tri), dv(vn), flat), mr.MeshRenderer(dv(v), dv(tri), dv(vn), flat)):
        with pytest.raises(RuntimeError, match="singular"):
            renderer.render(singular, proj, 8, 8)
    with pytest.raises(RuntimeError, match="not finite"):
        tf.NeTFRenderer(dv(v), dv(tri), dv(vn), flat).render(np.full((4, 4), np.nan, np.float32), proj, 8, 8)
