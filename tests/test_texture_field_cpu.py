"""CPU-side checks of the texture field (include/gd_texture.h, garmentdreamer_amd/texture_field.py): the production layout
is the pinned table; the REFERENCE (tests/texture_reference.py) is pinned itself, its vectorised form against the plain
loops and against its explicit backward, its float64 autograd gradients against central differences; the header's
entries are exported, bound and validate their arguments without a GPU; the documented errors."""
import os
import re

import numpy as np
import pytest
import torch

from tests import texture_reference as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_production_layout_is_the_pinned_table():
    from garmentdreamer_amd import texture_field as tf
    lay = tf.grid_layout()
    want_res = [16, 22, 28, 37, 49, 64, 85, 112, 148, 195, 256, 338, 446, 589, 777, 1024]
    want_size = [4096, 10648, 21952, 50656, 117656, 262144] + [524288] * 10
    assert lay.num_levels == 16 and lay.res.tolist() == want_res and lay.size.tolist() == want_size
    assert lay.dense.tolist() == [True] * 6 + [False] * 10
    assert lay.offset.tolist() == np.concatenate(([0], np.cumsum(want_size))).tolist()
    assert lay.num_entries == 5_710_032 and lay.num_params == 11_420_064 and lay.output_dim == 32
    assert abs(lay.num_params * 4 / 1e6 - 45.7) < 0.05
    assert lay.scale.dtype == np.float32 and float(lay.scale[0]) == 15.0 and float(lay.scale[15]) == 1023.0
    assert float(lay.scale[5]) == 63.0                       # exactly on the ceil boundary: res = 64, not 65
    # the reference's constructor arguments give the same table, and so does the test reference's own statement
    enc = tf.HashGridEncoder()
    assert enc.output_dim == 32 and enc.input_dim == 3 and tuple(enc.params.shape) == (11_420_064,)
    params = enc.params.detach()
    assert float(params.abs().max()) <= 1e-4 and float(params.min()) < -9e-5 and float(params.max()) > 9e-5
    ref = tref.layout()
    for key in ("scale", "res", "size", "offset", "dense"):
        assert np.array_equal(ref[key], getattr(enc.layout, key)), key
    s = lay.struct()
    assert s.num_levels == 16 and list(s.res) == want_res and list(s.size) == want_size and s.offset[16] == 5_710_032


def test_small_layouts():
    from garmentdreamer_amd import texture_field as tf
    a = tf.grid_layout(4, 3, 2.0, 8)                         # the encoder-only test layout
    assert a.scale.tolist() == [2.0, 5.0, 11.0, 23.0] and a.res.tolist() == [3, 6, 12, 24]
    assert a.size.tolist() == [32, 216, 256, 256]            # 27 -> 32 (round up to 8), 216 dense, two hashed at 2^8
    assert a.dense.tolist() == [True, True, False, False] and a.offset.tolist() == [0, 32, 248, 504, 760]
    b = tf.grid_layout(16, 2, 1.3, 10)                       # the fused test layout
    assert b.output_dim == 32 and b.res[0] == 2 and b.size[0] == 8
    assert b.dense.tolist() == [True] * 7 + [False] * 9 and b.size[6] == 1000 and (b.size[7:] == 1024).all()
    for lay, kw in ((a, dict(num_levels=4, base_resolution=3, per_level_scale=2.0, log2_hashmap_size=8)),
                    (b, dict(num_levels=16, base_resolution=2, per_level_scale=1.3, log2_hashmap_size=10))):
        ref = tref.layout(**kw)
        for key in ("scale", "res", "size", "offset", "dense"):
            assert np.array_equal(ref[key], getattr(lay, key)), key
    for bad in (dict(num_levels=0), dict(num_levels=17), dict(log2_hashmap_size=25), dict(base_resolution=0),
                dict(per_level_scale=0.5)):
        with pytest.raises(ValueError):
            tf.grid_layout(**bad)


def _small_problem(dtype, n=40, seed=3):
    lay = tref.layout(num_levels=16, base_resolution=2, per_level_scale=1.3, log2_hashmap_size=10)
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape, s=1.0: ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * s).to(dtype)
    p = dict(grid=rnd(int(lay["offset"][-1]) * 2), w1=rnd(32, 32, s=0.3), b1=rnd(32, s=0.3), w2=rnd(3, 32, s=0.3),
             b2=rnd(3, s=0.3))
    x = tref.sample_points(n, seed=seed)
    mask = torch.ones(n, dtype=torch.uint8)
    mask[4::7] = 0
    return lay, p, x, mask, rnd(n, 3)


def test_reference_forms_agree():
    """vectorised against plain loops: the same IEEE operations in the same order, so bit-equal in both dtypes; the explicit
    backward against autograd of the vectorised forward: the same terms in another order, a few ulp of float64"""
    for kw in (dict(num_levels=4, base_resolution=3, per_level_scale=2.0, log2_hashmap_size=8),
               dict(num_levels=16, base_resolution=2, per_level_scale=1.3, log2_hashmap_size=10)):
        lay = tref.layout(**kw)
        x = tref.sample_points(30, seed=1)
        mask = torch.ones(30, dtype=torch.uint8)
        mask[2] = 0
        for dtype in (torch.float32, torch.float64):
            grid = torch.from_numpy(np.random.RandomState(2).uniform(-1, 1, int(lay["offset"][-1]) * 2)).to(dtype)
            enc = tref.encode(x, grid, lay, mask)
            assert enc.dtype == dtype and torch.isfinite(enc).all()
            assert not enc[2].any() and not enc[15].any() and not enc[17].any()       # masked, NaN row, inf row
            assert enc[11].any() and enc[13].any()                                    # -1.5 and 2.0 are defined
            for l in range(lay["num_levels"]):
                assert torch.equal(enc[:, 2 * l:2 * l + 2], tref.encode_level_looped(x, grid, lay, l, mask)), (dtype, l)
    lay, p, x, mask, dcolor = _small_problem(torch.float64)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    color = tref.field(x, leaves["grid"], leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"], lay, mask)
    (color * dcolor).sum().backward()
    for order in (None, torch.arange(x.shape[0]).flip(0)):
        got = tref.field_backward(x, p["grid"], p["w1"], p["b1"], p["w2"], p["b2"], lay, dcolor, mask, order)
        assert float((got["color"] - color.detach()).abs().max()) <= 1e-15
        for k in ("grid", "w1", "b1", "w2", "b2"):
            auto = leaves[k].grad
            assert float(auto.abs().max()) > 0
            assert float((got["d" + k].reshape(auto.shape) - auto).abs().max()) <= 1e-14 * float(auto.abs().max()), k


def test_reference_autograd_gradients_agree_with_central_differences():
    lay, p, x, mask, dcolor = _small_problem(torch.float64, n=24)

    def loss(q):
        return float((tref.field(x, q["grid"], q["w1"], q["b1"], q["w2"], q["b2"], lay, mask) * dcolor).sum())

    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    (tref.field(x, leaves["grid"], leaves["w1"], leaves["b1"], leaves["w2"], leaves["b2"], lay, mask) * dcolor).sum().backward()
    rng = np.random.RandomState(0)
    # 1e-6 steps of quantities of order 1 in float64: truncation ~1e-12, rounding ~1e-16 |L| / 1e-6 ~ 1e-9 of the largest
    # gradient.  (A step across a ReLU kink would show as an error of order 1; none of these inputs sits within 1e-6 of one.)
    for k in ("grid", "w1", "b1", "w2", "b2"):
        grad = leaves[k].grad.reshape(-1).numpy()
        touched = np.flatnonzero(grad)
        assert touched.size > 0
        picks = touched if touched.size <= 40 else rng.choice(touched, 40, replace=False)
        if k == "grid":                                   # an untouched entry has gradient exactly 0 both ways
            picks = np.concatenate((picks, np.flatnonzero(grad == 0)[:3]))
        worst = 0.0
        for i in picks:
            hi, lo = {a: b.clone() for a, b in p.items()}, {a: b.clone() for a, b in p.items()}
            hi[k].view(-1)[i] += 1e-6
            lo[k].view(-1)[i] -= 1e-6
            worst = max(worst, abs((loss(hi) - loss(lo)) / 2e-6 - grad[i]))
        err = worst / np.abs(grad).max()
        print(k, "max |fd - autograd| / max |autograd|", err)
        assert err <= 1e-6, (k, err)


def test_texture_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gd_texture.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gd_texture_[a-z0-9_]+)\s*\(", text)))
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert len(declared) == 6
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_texture.h but not exported"
    assert sorted(_native.TEXTURE_SIGNATURES) == declared
    others = set(_native.SIGNATURES) | set(_native.SCENE_SIGNATURES) | set(_native.MESH_SIGNATURES) \
        | set(_native.MESH_DEFORM_SIGNATURES) | set(_native.MESH_GEOMETRY_SIGNATURES)
    assert not set(declared) & others
    import ctypes
    assert ctypes.sizeof(_native.TextureLayout) == 4 * (1 + 16 * 3 + 17)          # the header's struct, no padding
    assert L.gd_texture_field_backward_scratch_bytes(0) == 0 and L.gd_texture_field_backward_scratch_bytes(-4) == 0
    assert L.gd_texture_field_backward_scratch_bytes(1) >= 1155 * 4
    assert L.gd_texture_field_backward_scratch_bytes(1 << 30) <= 8 << 20          # the slab is bounded, whatever N


def _entries(L, lay, x=0x1000):
    """name -> (call(N, layout, pointers), number of pointers); the pointers in the order of the header, mask second"""
    return {
        "encode forward": (lambda N, s, p: L.gd_texture_encode_forward(None, N, p[0], p[1], p[2], s, p[3]), 4),
        "encode backward": (lambda N, s, p: L.gd_texture_encode_backward(None, N, p[0], p[1], p[2], s, p[3]), 4),
        "field forward": (lambda N, s, p: L.gd_texture_field_forward(None, N, p[0], p[1], p[2], s, *p[3:]), 8),
        "field backward": (lambda N, s, p: L.gd_texture_field_backward(None, N, p[0], p[1], p[2], s, *p[3:]), 15),
    }


def test_entries_validate_their_arguments():
    """-1 and a message before any device work (no GPU is touched: the stream is never used, no pointer is followed)"""
    from garmentdreamer_amd import _native
    from garmentdreamer_amd import texture_field as tf
    L = _native.lib()
    err = L.gd_texture_last_error
    lay = tf.grid_layout(16, 2, 1.3, 10)
    x = 0x1000                                     # a non-null, 8-byte aligned pointer that is never followed
    for name, (call, nptr) in _entries(L, lay).items():
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

        def broken(edit):
            s = lay.struct()
            edit(s)
            return call(5, s, good)

        def set_levels(v):
            return lambda s: setattr(s, "num_levels", v)

        def set_item(field, i, v):
            return lambda s: getattr(s, field).__setitem__(i, v)

        for what, edit in (("L = 0", set_levels(0)), ("L = 17", set_levels(17)), ("L = -1", set_levels(-1)),
                           ("size = 0", set_item("size", 3, 0)), ("size < 0", set_item("size", 0, -8)),
                           ("res = 0", set_item("res", 2, 0)), ("res < 0", set_item("res", 15, -1)),
                           ("equal offsets", set_item("offset", 4, lay.struct().offset[3])),
                           ("decreasing offsets", set_item("offset", 9, 5)),
                           ("offset[0] != 0", set_item("offset", 0, 8)),
                           ("offsets that skip entries", set_item("offset", 16, lay.struct().offset[16] + 8))):
            assert broken(edit) == -1 and b"layout" in err() and name.encode() in err(), (name, what)
        if name.startswith("field"):                                       # the fused path needs L F = 32
            short = tf.grid_layout(4, 3, 2.0, 8)
            assert call(5, short.struct(), good) == -1 and b"32" in err()
        if name != "encode backward":                                      # the grid is read as float2
            args = list(good)
            args[2] = x + 4
            assert call(5, lay.struct(), args) == -1 and b"aligned" in err()


def test_documented_errors():
    from garmentdreamer_amd import texture_field as tf
    small = tf.grid_layout(16, 2, 1.3, 10)
    enc = tf.HashGridEncoder.from_layout(small)
    fld = tf.TextureField(enc)
    assert fld.encoder is enc and [tuple(p.shape) for p in fld.mlp.parameters()] == [(32, 32), (32,), (3, 32), (3,)]
    x = torch.zeros(5, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        enc(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fld(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fld(x, mask=torch.ones(5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        fld.optimizer()
    with pytest.raises(RuntimeError, match="no CPU path"):
        tf.NeTFRenderer(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(3, 3), fld)
    with pytest.raises(NotImplementedError, match="smoothstep"):
        tf.HashGridEncoder(interpolation="smoothstep", log2_hashmap_size=4, num_levels=2)
    with pytest.raises(NotImplementedError):
        tf.HashGridEncoder(level_dim=4, log2_hashmap_size=4, num_levels=2)
    with pytest.raises(NotImplementedError):
        tf.HashGridEncoder(input_dim=2, log2_hashmap_size=4, num_levels=2)
    with pytest.raises(ValueError, match="bound"):
        enc(x, bound=2)
    with pytest.raises(ValueError, match="32"):
        tf.TextureField(tf.HashGridEncoder.from_layout(tf.grid_layout(4, 3, 2.0, 8)))
    groups = fld.get_params(0.01, 0.001)
    assert [g["lr"] for g in groups] == [0.01, 0.001]
    assert groups[0]["params"][0] is enc.params and len(groups[1]["params"]) == 4


def test_albedo_mlp_is_two_linears_with_blocked_weight_gradients():
    """float64 on the CPU: the same forward and gradients as the two ``nn.Linear`` to rounding, at row counts either side of
    the block (a few ulp: the blocks only change the order of the sum); no rows give zero gradients"""
    from garmentdreamer_amd import texture_field as tf
    torch.manual_seed(0)
    mlp = tf.AlbedoMLP().double()
    for n in (0, 1, 127, 128, 129, 300):
        x = torch.randn(n, 32, dtype=torch.float64, requires_grad=True)
        x2 = x.detach().clone().requires_grad_(True)
        w = torch.randn(n, 3, dtype=torch.float64)
        mlp.zero_grad()
        (mlp(x) * w).sum().backward()
        got = [p.grad.clone() for p in mlp.parameters()]
        mlp.zero_grad()
        y2 = mlp.net[1](torch.relu(mlp.net[0](x2)))
        (y2 * w).sum().backward()
        assert torch.equal(mlp(x).detach(), y2.detach())
        assert float((x.grad - x2.grad).abs().max()) <= 1e-13 if n else x.grad.shape == (0, 32)
        for a, p in zip(got, mlp.parameters()):
            assert a.shape == p.grad.shape and float((a - p.grad).abs().max()) <= 1e-12 * max(1.0, float(p.grad.abs().max()))
