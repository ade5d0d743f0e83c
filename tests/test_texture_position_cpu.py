"""CPU-side checks of the texture field's gradient to the positions (include/gd_texture_position.h): the REFERENCE
(tests/texture_position_reference.py) is pinned itself, its closed form against autograd of the non-detached float64
encoding and against central differences; the header's entries are exported, bound in a table of their own and validate
their arguments without a GPU; the Python flag defaults to off and leaves the refusal in place."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import texture_position_reference as pref
from tests import texture_reference as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {"small": dict(num_levels=16, base_resolution=2, per_level_scale=1.3, log2_hashmap_size=10), "production": {}}


@functools.lru_cache(maxsize=None)
def _problem(name):
    """layout, float64 grid, the test plan's points, a mask, denc and autograd's dx of sum(enc * denc); read-only"""
    lay = tref.layout(**LAYOUTS[name])
    rng = np.random.RandomState(5)
    grid = torch.from_numpy(rng.uniform(-1, 1, int(lay["offset"][-1]) * 2))
    x = tref.sample_points(4096, seed=3)
    mask = torch.ones(4096, dtype=torch.uint8)
    mask[4::7] = 0
    denc = torch.from_numpy(rng.uniform(-1, 1, size=(4096, 2 * lay["num_levels"])))
    auto = {}
    for key, m in (("masked", mask), ("all", None)):
        leaf = x.double().requires_grad_(True)
        (pref.encode_autograd(leaf, grid, lay, m) * denc).sum().backward()
        auto[key] = leaf.grad
    return lay, grid, x, mask, denc, auto


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_autograd_encoding_is_the_reference_encoding(name):
    lay, grid, x, mask, _, _ = _problem(name)
    assert torch.equal(pref.encode_autograd(x.double(), grid, lay, mask), tref.encode(x, grid, lay, mask))
    g32 = grid.float()
    assert torch.equal(pref.encode_autograd(x, g32, lay, None), tref.encode(x, g32, lay, None))


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_closed_form_equals_autograd(name):
    """float64: the header's sum is autograd's gradient of the non-detached encoding up to the order of the additions"""
    lay, grid, x, mask, denc, auto = _problem(name)
    for key, m in (("masked", mask), ("all", None)):
        got = pref.position_gradient(x, grid, denc, lay, m)
        scale = float(auto[key].abs().max())
        err = float((got - auto[key]).abs().max()) / scale
        print(f"{name} {key}: max|closed - autograd| / max|autograd| {err:.3g}")
        assert scale > 0 and err <= 1e-13
        dead = ~tref.valid_rows(x, m)
        assert dead.any() and not got[dead].any() and not auto[key][dead].any()      # exactly 0
    f32 = pref.position_gradient(x, grid.float(), denc.float(), lay, mask)
    assert f32.dtype == torch.float32 and pref.rel(f32, auto["masked"]) <= 1e-4       # the float32 statement, same function


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_central_differences(name):
    """float64, step 1e-7 in x, at the points whose every fractional part is in [1e-3, 1 - 1e-3] (a step of 1e-7 in x is
    at most 1e-7 * 0.5 * 1023 in w: it stays in the cell).  The encoding is trilinear in the cell, so the truncation error
    of a central difference is zero up to the cubic term's 1e-14; rounding is ~1e-16 |L| / 1e-7 ~ 1e-9 of a gradient whose
    largest element is of order s_l: within 1e-6 of max|autograd|, the bound of the grid's central-difference test."""
    lay, grid, x, _, denc, auto = _problem(name)
    finite = torch.isfinite(x).all(dim=1)
    keep = pref.interior(x, lay, 1e-3)
    share = float(keep.sum()) / float(finite.sum())
    print(f"{name}: {int(keep.sum())} of {int(finite.sum())} finite points kept ({100 * share:.1f} %)")
    assert share >= 0.85
    xs, d = x[keep].double(), denc[keep]
    want = auto["all"][keep]
    step = 1e-7
    fd = torch.empty_like(want)
    for k in range(3):
        hi, lo = xs.clone(), xs.clone()
        hi[:, k] += step
        lo[:, k] -= step
        fd[:, k] = ((tref.encode(hi, grid, lay) - tref.encode(lo, grid, lay)) * d).sum(dim=1) / (hi[:, k] - lo[:, k])
    err = float((fd - want).abs().max()) / float(want.abs().max())
    print(f"{name}: max|fd - autograd| / max|autograd| {err:.3g}")
    assert err <= 1e-6


def test_derivative_on_a_cell_wall_is_the_upper_cell_s():
    """w_0 = 0 exactly (one level, s = 4, x_0 = -0.25: p_0 = 2): the forward chose the cell above the wall, and so does
    the gradient"""
    lay = tref.layout(num_levels=1, base_resolution=5, per_level_scale=1.0, log2_hashmap_size=10)
    s = float(lay["scale"][0])                      # 4
    x = torch.tensor([[(2 * (2.0 - 0.5) / s) - 1, 0.3, -0.2]], dtype=torch.float64)       # p_0 = 2 exactly
    grid = torch.from_numpy(np.random.RandomState(1).uniform(-1, 1, int(lay["offset"][-1]) * 2))
    denc = torch.tensor([[0.7, -0.4]], dtype=torch.float64)
    at = pref.position_gradient(x, grid, denc, lay)
    above = pref.position_gradient(x + torch.tensor([[1e-9, 0, 0]]), grid, denc, lay)
    below = pref.position_gradient(x - torch.tensor([[1e-9, 0, 0]]), grid, denc, lay)
    assert float((at[0, 0] - above[0, 0]).abs()) <= 1e-12 * float(at.abs().max())
    assert float((at[0, 0] - below[0, 0]).abs()) > 1e-3 * float(at.abs().max())       # the lower cell has another slope


def _declared():
    text = open(os.path.join(ROOT, "include", "gd_texture_position.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gd_texture_[a-z0-9_]+)\s*\(", text)))


def test_position_symbols_declared_exported_and_bound():
    from garmentdreamer_amd import _native
    declared = _declared()
    L = _native.lib()
    assert declared == ["gd_texture_encode_backward_pos", "gd_texture_field_backward_pos",
                        "gd_texture_field_backward_sorted_pos"]
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_texture_position.h but not exported"
        assert getattr(L, name).argtypes == _native.TEXTURE_POSITION_SIGNATURES[name][1]        # lib() bound the table
        assert _native.error_channel(name) == "gd_texture_last_error"
    assert sorted(_native.TEXTURE_POSITION_SIGNATURES) == declared
    assert not set(declared) & (set(_native.TEXTURE_SIGNATURES) | set(_native.TEXTURE_SORTED_SIGNATURES))


def _entries(L):
    """name -> (call(N, layout, pointers), number of pointers, index of the grid); the pointers in the header's order"""
    return {
        "encode backward pos": (lambda N, s, p: L.gd_texture_encode_backward_pos(None, N, p[0], p[1], p[2], s, *p[3:]), 5),
        "field backward pos": (lambda N, s, p: L.gd_texture_field_backward_pos(None, N, p[0], p[1], p[2], s, *p[3:]), 16),
        "field backward sorted pos": (lambda N, s, p: L.gd_texture_field_backward_sorted_pos(None, N, p[0], p[1], p[2], s,
                                                                                             *p[3:]), 18),
    }


def test_entries_validate_their_arguments():
    """-1 and a message before any device work (no GPU is touched: the stream is never used, no pointer is followed)"""
    from garmentdreamer_amd import _native
    from garmentdreamer_amd import texture_field as tf
    L = _native.lib()
    err = L.gd_texture_last_error
    lay = tf.grid_layout(16, 2, 1.3, 10)
    x = 0x1000                                     # non-null, 16-byte aligned, never followed
    for name, (call, nptr) in _entries(L).items():
        good = [x] * nptr
        assert call(0, lay.struct(), good) == 0, name                      # N == 0: nothing to do, nothing launched
        for N in (-1, -(1 << 31)):
            assert call(N, lay.struct(), good) == -1 and name.encode() in err() and b"N must" in err(), name
        for hole in range(nptr):
            args = list(good)
            args[hole] = None
            if hole == 1:                                                  # the mask may be null; N = 0 keeps it a dry run
                assert call(0, lay.struct(), args) == 0, name
                continue
            assert call(5, lay.struct(), args) == -1 and b"null" in err() and name.encode() in err(), (name, hole)
        for what, edit in (("L = 0", lambda s: setattr(s, "num_levels", 0)), ("L = 17", lambda s: setattr(s, "num_levels", 17)),
                           ("size = 0", lambda s: s.size.__setitem__(3, 0)), ("res = 0", lambda s: s.res.__setitem__(2, 0)),
                           ("decreasing offsets", lambda s: s.offset.__setitem__(9, 5)),
                           ("offset[0] != 0", lambda s: s.offset.__setitem__(0, 8))):
            s = lay.struct()
            edit(s)
            assert call(5, s, good) == -1 and b"layout" in err() and name.encode() in err(), (name, what)
        args = list(good)
        args[2] = x + 4                                                    # the grid is read as float2
        assert call(5, lay.struct(), args) == -1 and b"aligned" in err() and name.encode() in err()
        if name.startswith("field"):                                       # the fused path needs L F = 32
            assert call(5, tf.grid_layout(4, 3, 2.0, 8).struct(), good) == -1 and b"32" in err()
    call, nptr = _entries(L)["field backward sorted pos"]
    assert call((1 << 24) + 1, lay.struct(), [x] * nptr) == -1 and b"2^24" in err() and b"atomic path" in err()
    args = [x] * nptr
    args[14] = x + 8                                                       # denc is written as float4
    assert call(5, lay.struct(), args) == -1 and b"denc" in err() and b"aligned" in err()


def test_python_flag_defaults_to_off():
    from garmentdreamer_amd import texture_field as tf
    assert inspect.signature(tf.encode).parameters["position_gradient"].default is False
    assert inspect.signature(tf.field).parameters["position_gradient"].default is False
    small = tf.grid_layout(16, 2, 1.3, 10)
    assert tf.HashGridEncoder.from_layout(small).position_gradient is False
    assert tf.HashGridEncoder.from_layout(small, position_gradient=True).position_gradient is True
    assert tf.HashGridEncoder(log2_hashmap_size=4, num_levels=2).position_gradient is False
    assert tf.HashGridEncoder(log2_hashmap_size=4, num_levels=2, position_gradient=True).position_gradient is True
    enc = tf.HashGridEncoder.from_layout(small)
    assert tf.TextureField(enc).encoder.position_gradient is False            # None leaves the encoder's flag
    assert tf.TextureField(enc, position_gradient=True).encoder.position_gradient is True and enc.position_gradient is True
    assert tf.TextureField(enc, position_gradient=False).encoder.position_gradient is False
    assert enc.deterministic is False                                          # the other flag is not touched


def test_flag_off_still_refuses_and_cpu_tensors_have_no_path(monkeypatch):
    from garmentdreamer_amd import texture_field as tf
    small = tf.grid_layout(16, 2, 1.3, 10)
    for flag in (False, True):
        fld = tf.TextureField(tf.HashGridEncoder.from_layout(small), position_gradient=flag)
        x = torch.zeros(5, 3, requires_grad=True)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fld(x)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fld.encoder(x)
        with pytest.raises(RuntimeError, match="no CPU path"):
            tf.encode(x, fld.encoder.params, small, position_gradient=flag)
    # the decision itself, with the device check stepped over (there is no GPU tensor to hand it here)
    monkeypatch.setattr(tf, "require_gpu", lambda name, what, t, *a: t)
    x = torch.zeros(5, 3, requires_grad=True)
    for name in ("encode", "field"):
        with pytest.raises(NotImplementedError, match="positions are not implemented"):
            tf._points(name, x, None)
        with pytest.raises(NotImplementedError, match="positions are not implemented"):
            tf._points(name, x, None, False)
    kept, _ = tf._points("field", x, None, True)
    assert kept.requires_grad                                                  # autograd sees it
    with torch.no_grad():
        assert not tf._points("field", x, None)[0].requires_grad               # no grad mode: nothing to refuse
    assert not tf._points("field", x.detach(), None, True)[0].requires_grad    # needs none: detached as before
