"""GPU checks of the texture field's gradient to the positions (include/gd_texture_position.h; csrc/raster_texture.hip;
``position_gradient=True`` in garmentdreamer_amd/texture_field.py) against the CPU statement of its definition
(tests/texture_position_reference.py).

The stand-alone ``dx`` is compared bit for bit with the float32 statement.  Everything else is measured as
``max|g - g64| / max|g64|`` against float64, and the allowance is FOUR times the same error of the float32 statement on the
same input -- the rule of tests/test_texture_field_gpu.py; ``dx`` is one row per point, so there is no order of summation
over points to vary, and for ``dgrid`` the allowance is that test's: the largest error over its three orders.

Inputs: ``grid_layout(16, 2, 1.3, 10)`` (seven dense levels, nine hashed) at N = 1000, no multiple of 128 or 256, and the
production layout once at N = 4096; ``texture_reference.sample_points`` (coordinates outside [-1, 1], a NaN row, an inf row),
a mask with zeros, and ``mask=None``."""
import functools

import numpy as np
import pytest
import torch

from tests import texture_position_reference as pref
from tests import texture_reference as tref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {"small": (dict(num_levels=16, base_resolution=2, per_level_scale=1.3, log2_hashmap_size=10), 1000),
         "production": ({}, 4096)}
PARAMS = ("grid", "w1", "b1", "w2", "b2")
MLP_GRADS = ("dw1", "db1", "dw2", "db2")


def _tf():
    from garmentdreamer_amd import texture_field as tf
    return tf


def _lib():
    from garmentdreamer_amd import _native
    return _native.lib()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def _problem(name):
    """inputs on both sides, the float64 ``dx`` of both entries and their allowances; shared and treated as read-only"""
    kw, n = CASES[name]
    lay = tref.layout(**kw)
    layout = _tf().grid_layout(**kw) if kw else _tf().grid_layout()
    g = torch.Generator().manual_seed(n)
    rnd = lambda *shape, s=1.0: ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * s).float()
    p = dict(grid=rnd(int(lay["offset"][-1]) * 2), w1=rnd(32, 32, s=0.3), b1=rnd(32, s=0.3), w2=rnd(3, 32, s=0.3),
             b2=rnd(3, s=0.3))
    p64 = {k: v.double() for k, v in p.items()}
    x = tref.sample_points(n, seed=n)
    mask = torch.ones(n, dtype=torch.uint8)
    mask[4::7] = 0
    rng = np.random.RandomState(n)
    dcolor = torch.from_numpy(rng.uniform(-1, 1, size=(n, 3)).astype(np.float32))
    denc = torch.from_numpy(rng.uniform(-1, 1, size=(n, 32)).astype(np.float32))
    q = dict(name=name, n=n, lay=lay, layout=layout, p=p, p64=p64, x=x, mask=mask, dcolor=dcolor, denc=denc,
             gpu={k: v.to(DEV) for k, v in p.items()}, xg=x.to(DEV), maskg=mask.to(DEV), dcolorg=dcolor.to(DEV),
             dencg=denc.to(DEV))
    for key, m in (("masked", mask), ("all", None)):
        want = pref.position_gradient(x, p64["grid"], denc.double(), lay, m)
        f32 = pref.position_gradient(x, p["grid"], denc, lay, m)
        fwant = pref.field_position_gradient(x, p64, lay, dcolor, m)
        ff32 = pref.field_position_gradient(x, p, lay, dcolor, m)
        q[key] = dict(enc_want=want, enc_f32=f32, enc_allowed=4 * pref.rel(f32, want), field_want=fwant,
                      field_ref32=pref.rel(ff32, fwant), field_allowed=4 * pref.rel(ff32, fwant))
    return q


def _masks(q):
    return (("masked", q["mask"], q["maskg"]), ("all", None, None))


def _raw_encode_pos(q, maskg, dx=None):
    dx = torch.full((q["n"], 3), float("nan"), device=DEV) if dx is None else dx
    ret = _lib().gd_texture_encode_backward_pos(_stream(), q["n"], q["xg"].data_ptr(), _ptr(maskg),
                                                q["gpu"]["grid"].data_ptr(), q["layout"].struct(), q["dencg"].data_ptr(),
                                                dx.data_ptr())
    assert ret == 0, _lib().gd_texture_last_error()
    return dx


def _raw_field_pos(q, maskg, color, dx=None):
    """gd_texture_field_backward_pos into zeroed gradient buffers; ``dx`` and the scratch start as NaN"""
    L, n, g = _lib(), q["n"], q["gpu"]
    dx = torch.full((n, 3), float("nan"), device=DEV) if dx is None else dx
    bufs = [torch.zeros_like(g[k]) for k in PARAMS]
    scratch = torch.full((max(L.gd_texture_field_backward_scratch_bytes(n) // 4, 1),), float("nan"), device=DEV)
    ret = L.gd_texture_field_backward_pos(_stream(), n, q["xg"].data_ptr(), _ptr(maskg), g["grid"].data_ptr(),
                                          q["layout"].struct(), g["w1"].data_ptr(), g["b1"].data_ptr(), g["w2"].data_ptr(),
                                          g["b2"].data_ptr(), color.data_ptr(), q["dcolorg"].data_ptr(),
                                          *[b.data_ptr() for b in bufs], dx.data_ptr(), scratch.data_ptr())
    assert ret == 0, L.gd_texture_last_error()
    return dx, bufs


def _python(q, maskg, fused=True, deterministic=False, position_gradient=True):
    """(color, gradients by name, dx or None) through the Python ops: ``field`` or ``encode`` + a torch MLP"""
    tf = _tf()
    leaves = {k: v.clone().requires_grad_(True) for k, v in q["gpu"].items()}
    x = q["xg"].clone().requires_grad_(position_gradient)
    if fused:
        color = tf.field(x, *[leaves[k] for k in PARAMS], q["layout"], maskg, deterministic, position_gradient)
    else:
        enc = tf.encode(x, leaves["grid"], q["layout"], maskg, deterministic, position_gradient)
        color = torch.sigmoid(tref.mlp(enc, leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"]))
        live = torch.isfinite(q["xg"]).all(dim=1) if maskg is None else torch.isfinite(q["xg"]).all(dim=1) & (maskg != 0)
        color = color * live[:, None]
    color.backward(q["dcolorg"])
    return color.detach(), {"d" + k: leaves[k].grad for k in PARAMS}, x.grad


@pytest.mark.parametrize("name", sorted(CASES))
def test_stand_alone_dx_bit_equal_to_the_float32_statement(name):
    q = _problem(name)
    for key, m, mg in _masks(q):
        dx = _raw_encode_pos(q, mg)
        assert torch.isfinite(dx).all()                                     # NaN-filled before: every element written
        assert torch.equal(dx.cpu(), q[key]["enc_f32"]), (name, key)
        err = pref.rel(dx, q[key]["enc_want"])
        print(f"{name} {key}: stand-alone dx gpu {err:.3g} allowed {q[key]['enc_allowed']:.3g}")
        assert err <= q[key]["enc_allowed"]
        dead = ~tref.valid_rows(q["x"], m)
        assert dead.any() and not dx.cpu()[dead].any()                      # exactly 0
        assert torch.equal(_raw_encode_pos(q, mg), dx)                      # a pure function of its inputs
        assert torch.equal(_raw_encode_pos(q, mg, torch.full_like(dx, 7.0)), dx)   # written, not added
        # the Python op is the same call
        x = q["xg"].clone().requires_grad_(True)
        _tf().encode(x, q["gpu"]["grid"], q["layout"], mg, position_gradient=True).backward(q["dencg"])
        assert torch.equal(x.grad, dx)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_dx(name):
    q = _problem(name)
    tf = _tf()
    for key, m, mg in _masks(q):
        a = q[key]
        color = tf.field(q["xg"], *[q["gpu"][k] for k in PARAMS], q["layout"], mg)
        dx, _ = _raw_field_pos(q, mg, color)
        assert torch.isfinite(dx).all()
        err = pref.rel(dx, a["field_want"])
        print(f"{name} {key}: fused dx gpu {err:.3g} float32 statement {a['field_ref32']:.3g} allowed {a['field_allowed']:.3g}")
        assert err <= a["field_allowed"]
        dead = ~tref.valid_rows(q["x"], m)
        assert not dx.cpu()[dead].any()
        assert torch.equal(_raw_field_pos(q, mg, color)[0], dx)                             # reruns bit-identical
        assert torch.equal(_raw_field_pos(q, mg, color, torch.full_like(dx, 7.0))[0], dx)   # written, not added
        _, _, dx_py = _python(q, mg)
        assert torch.equal(dx_py, dx)
        _, _, dx_sorted = _python(q, mg, deterministic=True)
        assert torch.equal(dx_sorted, dx)                   # the sorted entry forms the same denc and the same sum
        _, _, dx_unfused = _python(q, mg, fused=False)
        scale = float(a["field_want"].abs().max())
        between = float((dx_unfused.cpu().double() - dx.cpu().double()).abs().max()) / scale
        print(f"{name} {key}: |fused - unfused| / max|g64| {between:.3g}, unfused against float64 "
              f"{pref.rel(dx_unfused, a['field_want']):.3g}")
        assert between <= a["field_allowed"] and pref.rel(dx_unfused, a["field_want"]) <= a["field_allowed"]


@functools.lru_cache(maxsize=None)
def _dgrid_allowance(name):
    """(float64 dgrid, 4 x the float32 reference's largest error over the three orders of test_texture_field_gpu.py)"""
    q = _problem(name)
    n, p, p64 = q["n"], q["p"], q["p64"]
    want = tref.field_backward(q["x"], *[p64[k] for k in PARAMS], q["lay"], q["dcolor"].double(), q["mask"])["dgrid"]
    orders = [(torch.from_numpy(np.random.RandomState(11).permutation(n)), False), (None, True),
              (torch.arange(n).flip(0), True)]
    ref32 = max(pref.rel(tref.field_backward(q["x"], *[p[k] for k in PARAMS], q["lay"], q["dcolor"], q["mask"], order,
                                             sequential)["dgrid"], want) for order, sequential in orders)
    return want, 4 * ref32


@pytest.mark.parametrize("name", sorted(CASES))
def test_flag_on_leaves_everything_else_as_it_was(name):
    q = _problem(name)
    mg = q["maskg"]
    want, allowed = _dgrid_allowance(name)
    for deterministic in (False, True):
        c_off, g_off, none = _python(q, mg, deterministic=deterministic, position_gradient=False)
        c_on, g_on, dx = _python(q, mg, deterministic=deterministic)
        assert none is None and dx is not None
        assert torch.equal(c_on, c_off)
        for k in MLP_GRADS:
            assert torch.equal(g_on[k], g_off[k]), (k, deterministic)
        if deterministic:
            assert torch.equal(g_on["dgrid"], g_off["dgrid"])
        e_on, e_off = pref.rel(g_on["dgrid"], want), pref.rel(g_off["dgrid"], want)
        print(f"{name} deterministic={deterministic}: dgrid with dx {e_on:.3g} without {e_off:.3g} allowed {allowed:.3g}")
        assert e_on <= allowed and e_off <= allowed
        assert torch.equal(g_on["dgrid"] == 0, g_off["dgrid"] == 0)       # the same entries are touched
    # the flag on and an x that needs no gradient: nothing is returned to it, and nothing else moves
    tf = _tf()
    leaves = [q["gpu"][k].clone().requires_grad_(True) for k in PARAMS]
    color = tf.field(q["xg"], *leaves, q["layout"], mg, True, True)
    color.backward(q["dcolorg"])
    _, g_off, _ = _python(q, mg, deterministic=True, position_gradient=False)
    assert torch.equal(color.detach(), c_off) and all(torch.equal(l.grad, g_off["d" + k]) for l, k in zip(leaves, PARAMS))


def test_flag_off_refuses_and_no_double_backward():
    q = _problem("small")
    tf = _tf()
    x = q["xg"].clone().requires_grad_(True)
    params = [q["gpu"][k] for k in PARAMS]
    with pytest.raises(NotImplementedError, match="positions are not implemented"):
        tf.field(x, *params, q["layout"])
    with pytest.raises(NotImplementedError, match="positions are not implemented"):
        tf.encode(x, params[0], q["layout"])
    with torch.no_grad():
        tf.field(x, *params, q["layout"])                                   # no grad mode: nothing to refuse
    fld = tf.TextureField(tf.HashGridEncoder.from_layout(q["layout"]), position_gradient=True).to(DEV)
    color = fld(x, q["maskg"])
    dx, = torch.autograd.grad(color.sum(), x, create_graph=True)
    assert not dx.requires_grad                             # a constant to autograd: nothing to differentiate again
    weight = torch.ones_like(color, requires_grad=True)     # dcolor that itself requires a gradient
    dx, = torch.autograd.grad((fld(x, q["maskg"]) * weight).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="twice"):
        dx.sum().backward()
