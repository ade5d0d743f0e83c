"""GPU checks of the texture sampling (csrc/raster_sample.hip, garmentdreamer_amd/texture_sample.py) against the numpy
statement of include/gd_sample.h (tests/sample_reference.py): bit equality wherever the header fixes every fp32 operation
(rast_db, the attribute derivatives, the pyramid, nearest and linear sampling and their gradients), the project's pixel
tolerance |d| <= 1e-5 + 1e-4 |x| against the float64 statement where the device's log2f enters (the mip filters), and the
gradient tolerance rtol 1e-3, atol 1e-6 x scale for their gradients.  Every raw call starts from output buffers full of
garbage.  Shapes are the smallest that can go wrong: textures 1 x 1, 4 x 8 (not square), 16 x 16 and 32 x 64, images of
5 x 7 pixels and renders of the tube at 17 rows x 33 columns, no multiple of any tile."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_reference as mref
from tests import mesh_scenes as scenes
from tests import sample_reference as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GARBAGE = 0x7F7F7F7F
TEXTURES = ((1, 1), (4, 8), (16, 16), (32, 64))                       # (Ht, Wt)
FILTERS, BOUNDARIES = sorted(sref.FILTERS), sorted(sref.BOUNDARIES)


def _ts():
    from garmentdreamer_amd import texture_sample
    return texture_sample


def _native():
    from garmentdreamer_amd import _native
    return _native


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _garbage(*shape, dtype=torch.float32):
    return torch.full(shape, GARBAGE, dtype=torch.int32, device=DEV).view(dtype) if dtype == torch.float32 \
        else torch.full(shape, GARBAGE, dtype=dtype, device=DEV)


def _up(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _call(name, *args):
    L = _native().lib()
    ret = getattr(L, name)(_stream(), *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])
    assert ret == 0, L.gd_mesh_last_error()


def _same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (bad.size, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


def _pixel_close(got, want):
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else got
    err = np.abs(got - want)
    tol = 1e-5 + 1e-4 * np.abs(want)
    print("pixel: max |d| = %.3g, worst d / tol = %.3g" % (err.max(), (err / tol).max()))
    assert got.shape == want.shape and (err <= tol).all(), (err.max(), np.unravel_index((err / tol).argmax(), err.shape))


# ---- rast_db and the attribute derivatives ----------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ("tube", "edge_cases"))
def test_rast_db_and_interpolate_da_equal_the_statement(scene):
    from garmentdreamer_amd import mesh_render as mr
    ts = _ts()
    if scene == "tube":
        (pos, tri), H, W = scenes.tube_clip(), 17, 33
    else:
        (pos, tri, _), H, W = scenes.edge_case_scene(), 48, 64
    p, t = _up(pos), _up(tri)
    rast = mr.rasterize(p, t, (H, W))
    V, F = pos.shape[0], tri.shape[0]
    db = _garbage(H, W, 4)
    _call("gd_sample_rast_db", V, F, H, W, rast, p, t, db)
    r = rast.cpu().numpy()
    hit = r[..., 3] > 0
    assert hit.sum() > 50 and (~hit).sum() > 50
    want = sref.rast_db(r, pos, tri)
    _same_bits(db, want)
    assert not db.cpu().numpy()[~hit].any() and np.abs(want[hit]).max() > 0
    assert torch.equal(ts.rast_derivatives(rast, p, t), db)
    assert torch.equal(ts.rast_derivatives(rast[None], p[None], t), db[None])
    rng = np.random.RandomState(1)
    for C in (1, 2, 3, 8):
        attr = rng.standard_normal((V, C)).astype(np.float32)
        da = _garbage(H, W, 2 * C)
        _call("gd_sample_interpolate_da", V, F, C, H, W, _up(attr), rast, db, t, da)
        _same_bits(da, sref.interpolate_da(attr, r, want, tri))
        assert not da.cpu().numpy()[~hit].any()
        assert torch.equal(ts.interpolate_derivatives(_up(attr), rast, db, t), da)
    with pytest.raises(ValueError, match="channels"):
        ts.interpolate_derivatives(torch.zeros(V, 9, device=DEV), rast, db, t)


# ---- the pyramid ------------------------------------------------------------------------------------------------------

def _padded(levels):
    C = levels[0].shape[2]
    out = np.zeros((int(sref.offsets(levels)[-1]), 4), dtype=np.float32)
    out[:, :C] = np.concatenate([lv.reshape(-1, C) for lv in levels])
    return out


@pytest.mark.parametrize("shape", TEXTURES, ids=lambda s: "%dx%d" % s)
def test_build_mips_equals_the_statement(shape):
    ts = _ts()
    rng = np.random.RandomState(shape[1])
    for C in (1, 3, 4):
        tex = rng.uniform(0, 1, shape + (C,)).astype(np.float32)
        for top in (None, 1, 0):
            levels = sref.build_mips(tex, top)
            lay = ts.pyramid_layout(shape[0], shape[1], top)
            buf = _garbage(lay.offset[lay.levels], 4)
            _call("gd_sample_build_mips", C, _up(tex), lay, buf)
            _same_bits(buf, _padded(levels))
            mip = ts.build_mipmaps(_up(tex), top)
            assert torch.equal(mip.buffer, buf) and list(mip.shapes) == [lv.shape[:2] for lv in levels]
            assert list(mip.offsets) == sref.offsets(levels).tolist()
    u8 = rng.randint(0, 256, shape + (3,)).astype(np.uint8)
    _same_bits(ts.build_mipmaps(_up(u8)).buffer, _padded(sref.build_mips(u8.astype(np.float32) / np.float32(255))))


def test_build_mipmaps_refuses_what_it_cannot_halve():
    ts = _ts()
    with pytest.raises(RuntimeError, match="power-of-two"):
        ts.build_mipmaps(torch.zeros(5, 7, 3, device=DEV))
    assert ts.build_mipmaps(torch.zeros(5, 7, 3, device=DEV), 0).layout.levels == 1
    with pytest.raises(ValueError, match="channels"):
        ts.build_mipmaps(torch.zeros(4, 4, 5, device=DEV))
    with pytest.raises(TypeError):
        ts.build_mipmaps(torch.zeros(4, 4, 3, device=DEV, dtype=torch.float64))


# ---- nearest and linear -----------------------------------------------------------------------------------------------

def _uv_5x7(Ht, Wt, seed):
    """[35,2]: the boundary values of both axes in two pairings, a NaN row, an infinite row and random rows"""
    rng = np.random.RandomState(seed)
    su = np.array([-0.25, 0.0, 0.5 / Wt, 1 - 0.5 / Wt, 1.0, 1.75])
    sv = np.array([-0.25, 0.0, 0.5 / Ht, 1 - 0.5 / Ht, 1.0, 1.75])
    uv = rng.uniform(-1.0, 2.0, (35, 2))
    uv[:6] = np.stack((su, sv), 1)
    uv[6:12] = np.stack((su, sv[::-1]), 1)
    uv[12:18, 0] = su
    uv[18:24, 1] = sv
    uv[24] = (np.nan, 0.3)
    uv[25] = (0.3, np.inf)
    return uv.astype(np.float32)


@pytest.mark.parametrize("shape", TEXTURES + ((5, 7),), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("filter_name", ("nearest", "linear"))
def test_nearest_and_linear_equal_the_statement(shape, filter_name):
    ts = _ts()
    rng = np.random.RandomState(7)
    fid = sref.FILTERS[filter_name]
    uv = _uv_5x7(shape[0], shape[1], 3)
    for C in (1, 3, 4):
        tex = rng.standard_normal(shape + (C,)).astype(np.float32)
        mip = ts.build_mipmaps(_up(tex), 0)
        for boundary_name in BOUNDARIES:
            want = sref.texture([tex], uv, None, fid, sref.BOUNDARIES[boundary_name])
            out = _garbage(35, C)
            _call("gd_sample_texture_forward", 35, C, fid, sref.BOUNDARIES[boundary_name], mip.layout, mip.buffer, _up(uv), None,
                  out)
            _same_bits(out, want)
            assert not want[24].any() and not want[25].any()
            pub = ts.texture(_up(tex), _up(uv).view(5, 7, 2), filter_mode=filter_name, boundary_mode=boundary_name)
            assert pub.shape == (5, 7, C) and torch.equal(pub.view(35, C), out)
            assert torch.equal(ts.texture(None, _up(uv), mip=mip, filter_mode=filter_name, boundary_mode=boundary_name), out)
    if filter_name == "linear":
        assert torch.equal(ts.texture(_up(tex), _up(uv)), ts.texture(_up(tex), _up(uv), filter_mode="linear"))   # 'auto'


# ---- the mip filters --------------------------------------------------------------------------------------------------

def _levelled(Ht, Wt, seed):
    """(uv [N,2], uv_da [N,4], levels [N]): isotropic footprints of 2^level texels with level = k + U(0.05, 0.45) and
    k + U(0.55, 0.95) for k = 0 .. L + 1 -- no pixel on the rounding step of linear-mipmap-nearest --, then all-zero rows
    (level 0) and huge ones (level L)"""
    rng = np.random.RandomState(seed)
    L = len(sref.pyramid_shapes(Ht, Wt)) - 1
    level = np.concatenate([k + rng.uniform(lo, hi, 4) for k in range(L + 2) for lo, hi in ((0.05, 0.45), (0.55, 0.95))])
    s = 2.0 ** level
    da = np.stack((s / Wt, np.zeros_like(s), np.zeros_like(s), s / Ht), axis=1)
    rot = rng.uniform(0, 2 * np.pi, s.shape[0])                                   # a rotation keeps the singular values
    c, sn = np.cos(rot), np.sin(rot)
    da = np.stack((da[:, 0] * c, -da[:, 0] * sn, da[:, 3] * sn, da[:, 3] * c), axis=1)
    da = np.concatenate((da, np.zeros((4, 4)), np.full((4, 4), 1e3) * rng.choice([-1, 1], (4, 4))))
    level = np.concatenate((level, np.zeros(4), np.full(4, L)))
    uv = (rng.randint(-512, 1536, (da.shape[0], 2)) / 1024.0)                     # a multiple of 1/1024: u Wl is exact
    return uv.astype(np.float32), da.astype(np.float32), np.clip(level, 0, L)


@pytest.mark.parametrize("shape", TEXTURES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("filter_name", ("linear-mipmap-nearest", "linear-mipmap-linear"))
def test_mip_filters_against_the_float64_statement(shape, filter_name):
    ts = _ts()
    rng = np.random.RandomState(5)
    fid = sref.FILTERS[filter_name]
    uv, da, level = _levelled(shape[0], shape[1], 9)
    L = len(sref.pyramid_shapes(*shape)) - 1
    assert np.abs(sref.mip_level(da, shape[0], shape[1], L, np.float64) - level).max() < 1e-4
    N = uv.shape[0]
    for C in (1, 3, 4):
        tex = rng.uniform(0, 1, shape + (C,)).astype(np.float32)
        mip = ts.build_mipmaps(_up(tex))
        levels64 = sref.build_mips(tex, None, np.float64)
        for boundary_name in BOUNDARIES:
            bid = sref.BOUNDARIES[boundary_name]
            out = _garbage(N, C)
            _call("gd_sample_texture_forward", N, C, fid, bid, mip.layout, mip.buffer, _up(uv), _up(da), out)
            _pixel_close(out, sref.texture(levels64, uv, da, fid, bid, np.float64))
            pub = ts.texture(_up(tex), _up(uv), _up(da), filter_mode=filter_name, boundary_mode=boundary_name)
            assert torch.equal(pub, out)
    if filter_name == "linear-mipmap-linear":
        assert torch.equal(ts.texture(_up(tex), _up(uv), _up(da), boundary_mode=boundary_name), pub)              # 'auto'
        one = ts.texture(_up(tex), _up(uv), _up(da), max_mip_level=1, boundary_mode="clamp")
        _pixel_close(one, sref.texture(sref.build_mips(tex, 1, np.float64), uv, da, fid, sref.CLAMP, np.float64))
    with pytest.raises(ValueError, match="needs uv_da"):
        ts.texture(_up(tex), _up(uv), filter_mode=filter_name)


def test_unknown_modes_and_odd_sizes_raise():
    ts = _ts()
    tex, uv = torch.zeros(4, 4, 3, device=DEV), torch.zeros(5, 2, device=DEV)
    with pytest.raises(ValueError, match="filter_mode"):
        ts.texture(tex, uv, filter_mode="cubic")
    with pytest.raises(ValueError, match="boundary_mode"):
        ts.texture(tex, uv, boundary_mode="zero")
    with pytest.raises(RuntimeError, match="power-of-two"):
        ts.texture(torch.zeros(5, 7, 3, device=DEV), uv, torch.zeros(5, 4, device=DEV))
    with pytest.raises(NotImplementedError, match="uv"):
        ts.texture(tex, uv.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="uv"):
        ts.texture(tex, uv, torch.zeros(5, 4, device=DEV, requires_grad=True))


def test_a_constant_texture_samples_to_the_constant():
    ts = _ts()
    half = np.float32(0.5)
    for shape in TEXTURES:
        uv, da, _ = _levelled(shape[0], shape[1], 2)
        uv = np.concatenate((uv, _uv_5x7(shape[0], shape[1], 4)[:24]))
        da = np.concatenate((da, np.resize(da, (24, 4))))
        tex = torch.full(shape + (3,), 0.5, device=DEV)
        for filter_name in FILTERS:
            for boundary_name in BOUNDARIES:
                out = ts.texture(tex, _up(uv), _up(da), filter_mode=filter_name, boundary_mode=boundary_name).cpu().numpy()
                assert np.abs(out - half).max() <= 2 * np.spacing(half), (shape, filter_name, boundary_name)


# ---- the gradient to the texture --------------------------------------------------------------------------------------

def _backward_case(shape, filter_name, C, seed):
    uv, da, _ = _levelled(shape[0], shape[1], seed)
    uv = np.concatenate((uv, _uv_5x7(shape[0], shape[1], seed + 1)))               # boundary values, NaN and inf rows
    da = np.concatenate((da, np.resize(da, (35, 4))))
    rng = np.random.RandomState(seed + 2)
    dout = rng.standard_normal((uv.shape[0], C)).astype(np.float32)
    top = None if sref.FILTERS[filter_name] >= sref.LINEAR_MIPMAP_NEAREST else 0
    return uv, da, dout, top


def _raw_backward(ts, shape, C, uv, da, dout, fid, bid, top, dtex):
    lay = ts.pyramid_layout(shape[0], shape[1], top)
    return ts.texture_backward(lay, C, _up(uv), _up(da), _up(dout), fid, bid, dtex)


@pytest.mark.parametrize("shape", TEXTURES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("filter_name", FILTERS)
def test_texture_backward(shape, filter_name):
    ts = _ts()
    fid = sref.FILTERS[filter_name]
    for C, boundary_name in ((3, "wrap"), (3, "clamp"), (1, "clamp"), (4, "wrap")):
        bid = sref.BOUNDARIES[boundary_name]
        uv, da, dout, top = _backward_case(shape, filter_name, C, 20 + C)
        shapes = sref.pyramid_shapes(shape[0], shape[1], top)
        zero = np.zeros(shape + (C,), dtype=np.float32)
        got = _raw_backward(ts, shape, C, uv, da, dout, fid, bid, top, _up(zero))
        if fid < sref.LINEAR_MIPMAP_NEAREST:
            _same_bits(got, sref.texture_backward(shapes, uv, da, dout, fid, bid, zero))         # the sequential sum
        else:
            want = sref.texture_backward(shapes, uv, da, dout, fid, bid, zero.astype(np.float64), np.float64)
            err = np.abs(got.cpu().numpy().astype(np.float64) - want)
            tol = 1e-6 * np.abs(want).max() + 1e-3 * np.abs(want)
            print("gradient: max |d| = %.3g, worst d / tol = %.3g" % (err.max(), (err / tol).max()))
            assert (err <= tol).all()
        # two runs are bit-identical
        again = _raw_backward(ts, shape, C, uv, da, dout, fid, bid, top, _up(zero))
        assert torch.equal(got.view(torch.int32), again.view(torch.int32))
        # a dtex that holds values is added to
        base = np.random.RandomState(3).standard_normal(shape + (C,)).astype(np.float32)
        added = _raw_backward(ts, shape, C, uv, da, dout, fid, bid, top, _up(base)).cpu().numpy()
        g = got.cpu().numpy()
        _same_bits(added, np.where(g != 0, base + g, base))


def test_texels_no_item_reaches_keep_their_bits():
    ts = _ts()
    shape, C = (16, 16), 3
    rng = np.random.RandomState(8)
    uv = rng.uniform(0.1, 0.4, (35, 2)).astype(np.float32)                          # a corner of the texture only
    dout = rng.standard_normal((35, C)).astype(np.float32)
    pattern = np.array([0x7FC12345, 0x80000000, GARBAGE, 0xFF800000], dtype=np.uint32)       # a NaN payload, -0, ...
    base = np.resize(pattern, shape + (C,)).view(np.float32)
    for filter_name in ("nearest", "linear"):
        fid = sref.FILTERS[filter_name]
        want = sref.texture_backward([shape], uv, None, dout, fid, sref.CLAMP, np.zeros(shape + (C,), np.float32))
        untouched = want == 0
        assert untouched.sum() > 100 and (~untouched).sum() > 20
        got = ts.texture_backward(ts.pyramid_layout(16, 16, 0), C, _up(uv), None, _up(dout), fid, sref.CLAMP,
                                  _up(base.copy())).cpu().numpy()
        assert np.array_equal(got.view(np.uint32)[untouched], base.view(np.uint32)[untouched])


@pytest.mark.parametrize("filter_name", ("linear", "linear-mipmap-linear"))
def test_autograd_reaches_the_texture(filter_name):
    ts = _ts()
    shape, C = (16, 16), 3
    fid = sref.FILTERS[filter_name]
    uv, da, dout, top = _backward_case(shape, filter_name, C, 31)
    tex = torch.rand(shape + (C,), device=DEV, requires_grad=True)
    want = _raw_backward(ts, shape, C, uv, da, dout, fid, sref.WRAP, top, torch.zeros(shape + (C,), device=DEV))
    out = ts.texture(tex, _up(uv), _up(da), filter_mode=filter_name)
    (out * _up(dout)).sum().backward()
    assert torch.equal(tex.grad, want)
    # through a pyramid built once: the gradient goes to the tensor it was built from
    src = tex.detach().clone().requires_grad_(True)
    mip = ts.build_mipmaps(src, top)
    (ts.texture(None, _up(uv), _up(da), mip=mip, filter_mode=filter_name) * _up(dout)).sum().backward()
    assert torch.equal(src.grad, want)
    with torch.no_grad():
        assert not ts.texture(tex, _up(uv), _up(da), filter_mode=filter_name).requires_grad


# ---- the textured render ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _export(folder):
    """the tube with a chart atlas at 256 x 256 and a seeded random albedo with the charts padded, written and read back"""
    from garmentdreamer_amd import mesh_render as mr
    from garmentdreamer_amd import texture_atlas as ta
    from garmentdreamer_amd import texture_bake as tb
    ts = _ts()
    v, tri, vn = scenes.tube()
    vt, ft, info = ta.chart_atlas(_up(v), _up(tri), 256)
    pos = torch.cat((vt * 2.0 - 1.0, torch.zeros_like(vt[:, :1]), torch.ones_like(vt[:, :1])), dim=1).contiguous()
    mask = mr.rasterize(pos, ft, (256, 256))[..., 3] > 0
    image = torch.from_numpy(np.random.RandomState(12).uniform(0, 1, (256, 256, 3)).astype(np.float32)).to(DEV)
    albedo = tb.uv_padding(image, mask, 4)
    paths = tb.write_textured_obj(folder + "/tube.obj", v, tri, vt, ft, albedo)
    back = ts.load_textured_obj(paths[0])
    assert np.array_equal(back[2].astype(np.float32), vt.cpu().numpy()) and np.array_equal(back[3], ft.cpu().numpy())
    assert np.array_equal(back[4], albedo.cpu().numpy()) and np.array_equal(back[1], tri)
    return back, vn, {}


@pytest.fixture(scope="module")
def export(tmp_path_factory):
    return _export(str(tmp_path_factory.mktemp("textured")))


def _camera():
    return scenes.look_at_pose(scenes.CAMPOS), scenes.perspective(scenes.FOVY)


def _positions(ts, v, pose, proj):
    """(pos, v_cam) as the package forms them: the two 4 x 4 products are torch's, and the statement starts from THEIR bits,
    after a check that they are the right positions"""
    v_cam, pos, _ = (t.cpu().numpy() for t in ts.clip_positions(_up(v), pose, proj))
    want_pos, want_cam = scenes.clip_positions(v, pose, proj)
    assert np.allclose(pos, want_pos, rtol=1e-5, atol=1e-6) and np.allclose(v_cam, want_cam, rtol=1e-5, atol=1e-6)
    return pos, v_cam


@pytest.mark.parametrize("resolution", ((17, 33), (64, 64)), ids=lambda r: "%dx%d" % r)
@pytest.mark.parametrize("filter_name,boundary_name", (("linear", "clamp"), ("linear-mipmap-linear", "wrap")))
def test_render_mesh_equals_the_statement(export, resolution, filter_name, boundary_name):
    from garmentdreamer_amd import mesh_render as mr
    ts = _ts()
    (v, f, vt, ft, albedo), vn, cache = export
    H, W = resolution
    pose, proj = _camera()
    v32 = v.astype(np.float32)
    out = ts.render_mesh(_up(v32), _up(f, torch.int32), vt, ft, _up(albedo), _up(vn), pose, proj, H, W, bg_color=1,
                         texture_filter=filter_name, boundary_mode=boundary_name)
    pos, v_cam = _positions(ts, v32, pose, proj)
    want = sref.render_mesh(mref, pos, v_cam, f.astype(np.int32), vt.astype(np.float32), ft, albedo, vn, pose, H, W,
                            filter_name, boundary_name, cache=cache)
    assert sorted(out) == ["alpha", "depth", "image", "normal", "viewcos"]
    assert (want["alpha"] > 0).sum() > 40 and ((want["alpha"] > 0) & (want["alpha"] < 1)).sum() > 5
    for key in sorted(out):
        assert tuple(out[key].shape) == want[key].shape == (H, W, 3 if key in ("image", "normal") else 1), key
        print(key, end=" ")
        _pixel_close(out[key], want[key])
    inside = want["alpha"][..., 0] == 1
    assert np.ptp(out["image"].cpu().numpy()[inside]) > 0.2                         # the albedo shows
    # alpha, depth and normal are those of the field renderer for the same camera
    other = mr.MeshRenderer(_up(v32), _up(f, torch.int32), _up(vn), lambda x: torch.zeros_like(x)).render(pose, proj, H, W)
    for key in ("alpha", "depth", "normal"):
        assert torch.equal(out[key], other[key]), key


def test_render_mesh_vertex_colours_normals_and_ssaa(export):
    from garmentdreamer_amd import mesh_geometry as mg
    ts = _ts()
    (v, f, vt, ft, albedo), vn, cache = export
    H, W = 17, 33
    pose, proj = _camera()
    v32, f32 = v.astype(np.float32), f.astype(np.int32)
    vc = np.random.RandomState(6).uniform(0, 1, v32.shape).astype(np.float32)
    out = ts.render_mesh(_up(v32), _up(f32), None, None, None, _up(vn), pose, proj, H, W, bg_color=0.25, vc=_up(vc))
    pos, v_cam = _positions(ts, v32, pose, proj)
    want = sref.render_mesh(mref, pos, v_cam, f32, None, None, None, vn, pose, H, W, "linear", "wrap", bg=0.25, vc=vc,
                            cache=cache)
    for key in sorted(out):
        print(key, end=" ")
        _pixel_close(out[key], want[key])
    # vn=None: the package's vertex normals
    geo = mg.build_geometry(_up(f32), num_vertices=v32.shape[0], device=DEV)
    own = mg.normals(_up(v32), geo)[1]
    a = ts.render_mesh(_up(v32), _up(f32), vt, ft, _up(albedo), None, pose, proj, H, W)
    b = ts.render_mesh(_up(v32), _up(f32), vt, ft, ts.build_mipmaps(_up(albedo)), own, pose, proj, H, W)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    with pytest.raises(ValueError, match="ssaa"):
        ts.render_mesh(_up(v32), _up(f32), vt, ft, _up(albedo), _up(vn), pose, proj, H, W, ssaa=2)
    # the gradient of an image loss reaches the albedo
    tex = (_up(albedo).float() / 255.0).requires_grad_(True)
    ts.render_mesh(_up(v32), _up(f32), vt, ft, tex, _up(vn), pose, proj, H, W)["image"].sum().backward()
    assert tex.grad.shape == tex.shape and torch.isfinite(tex.grad).all() and (tex.grad != 0).sum() > 100
