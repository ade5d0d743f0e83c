"""What can be said about the texture sampling without a GPU (include/gd_sample.h, garmentdreamer_amd/texture_sample.py,
export.load_image_rgb): the bindings against the header, every entry's argument validation (which returns before the
device is touched), the numpy statement of tests/sample_reference.py against facts it does not restate -- central
differences of the unsnapped (u, v), the singular values of numpy.linalg.svd, the adjoint identity -- the PNG reader
against files assembled here with zlib, and the round trip of a textured .obj."""
import ctypes
import os
import re
import struct
import zlib

import numpy as np
import pytest

from tests import mesh_reference as mref
from tests import mesh_scenes as scenes
from tests import sample_reference as sref

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "gd_sample.h")


def _native():
    from garmentdreamer_amd import _native
    return _native


def _layout(H, W, level):
    n = _native()
    out = n.SamplePyramid()
    assert n.lib().gd_sample_pyramid_layout(H, W, level, ctypes.byref(out)) == 0, n.lib().gd_mesh_last_error()
    return out


# ---- signatures and argument validation -------------------------------------------------------------------------------

def test_the_bindings_cover_the_header():
    n = _native()
    header = open(HEADER).read()
    declared = sorted(re.findall(r"^int (gd_sample_\w+)\(", header, flags=re.M))
    assert declared == sorted(n.SAMPLE_SIGNATURES) and len(declared) == 9
    L = n.lib()
    for name in declared:
        assert getattr(L, name).argtypes == n.SAMPLE_SIGNATURES[name][1]
        assert n.error_channel(name) == "gd_mesh_last_error"
        assert name not in n.MESH_SIGNATURES
        count = len(re.search(name + r"\((.*?)\);", header, flags=re.S).group(1).split(","))
        assert count == len(n.SAMPLE_SIGNATURES[name][1]), name
    for macro, value in (("MAX_SIDE", n.SAMPLE_MAX_SIDE), ("MAX_LEVELS", n.SAMPLE_MAX_LEVELS),
                         ("MAX_CHANNELS", n.SAMPLE_MAX_CHANNELS), ("TEXEL", n.SAMPLE_TEXEL)):
        assert int(re.search(rf"#define GD_SAMPLE_{macro} (\d+)", header).group(1)) == value
    for name, value in list(n.SAMPLE_FILTERS.items()) + list(n.SAMPLE_BOUNDARIES.items()):
        macro = "GD_SAMPLE_" + name.upper().replace("-", "_")
        assert int(re.search(rf"#define {macro} (\d+)", header).group(1)) == value
        assert (sref.FILTERS.get(name, sref.BOUNDARIES.get(name))) == value
    assert [L.gd_sample_taps(i) for i in range(5)] == [1, 4, 4, 8, -1] and sref.TAPS == {0: 1, 1: 4, 2: 4, 3: 8}
    assert "unverified" in header.lower() and "nvdiffrast" in header


def test_the_source_is_built_without_contraction():
    from garmentdreamer_amd import _build
    assert ("raster_sample.hip", ["-ffp-contract=off"]) in _build.RASTER_SOURCES


def test_the_layout_is_the_statement_s():
    for H, W, level in ((1, 1, -1), (4, 8, -1), (16, 16, -1), (32, 64, -1), (32, 64, 1), (16, 16, 99), (5, 7, 0), (16384, 16384, -1)):
        lay = _layout(H, W, level)
        shapes = sref.pyramid_shapes(H, W, None if level < 0 else level)
        assert lay.levels == len(shapes)
        assert [(lay.height[l], lay.width[l]) for l in range(lay.levels)] == shapes
        off = np.concatenate(([0], np.cumsum([h * w for h, w in shapes])))
        assert [lay.offset[l] for l in range(lay.levels + 1)] == off.tolist()
    n = _native()
    out = n.SamplePyramid()
    L = n.lib()
    for H, W, level, piece in ((5, 7, -1, "power-of-two"), (12, 16, 1, "power-of-two"), (0, 4, 0, "1..16384"),
                               (4, 16385, 0, "1..16384")):
        assert L.gd_sample_pyramid_layout(H, W, level, ctypes.byref(out)) == -1
        assert piece in L.gd_mesh_last_error().decode()
    assert L.gd_sample_pyramid_layout(4, 4, 0, None) == -1


P = 0x1000          # a non-null address no entry may dereference: every call below must return before the device is touched


def _bad_calls():
    n = _native()
    good, odd = _layout(16, 16, -1), _layout(5, 7, 0)
    broken = _layout(16, 16, -1)
    broken.offset[1] = 255
    F, B = n.SAMPLE_FILTERS, n.SAMPLE_BOUNDARIES
    mip, lin, wrap = F["linear-mipmap-linear"], F["linear"], B["wrap"]
    return {
        "gd_sample_rast_db": [((None, 3, 1, 4, 4, None, P, P, P), "null"), ((None, 3, 1, 4, 4, P, P, P, None), "null"),
                              ((None, 0, 1, 4, 4, P, P, P, P), "V must"), ((None, 3, 0, 4, 4, P, P, P, P), "V must"),
                              ((None, 3, 1 << 24, 4, 4, P, P, P, P), "V must"), ((None, 3, 1, 0, 4, P, P, P, P), "H and W")],
        "gd_sample_interpolate_da": [((None, 3, 1, 2, 4, 4, P, P, None, P, P), "null"),
                                     ((None, 3, 1, 0, 4, 4, P, P, P, P, P), "1..8"),
                                     ((None, 3, 1, 9, 4, 4, P, P, P, P, P), "1..8"),
                                     ((None, 3, 1, 2, 4, -1, P, P, P, P, P), "H and W")],
        "gd_sample_build_mips": [((None, 3, None, good, P), "null"), ((None, 3, P, good, None), "null"),
                                 ((None, 0, P, good, P), "1..4"), ((None, 5, P, good, P), "1..4"),
                                 ((None, 3, P, broken, P), "pyramid")],
        "gd_sample_texture_forward": [((None, 8, 3, lin, wrap, good, None, P, None, P), "null"),
                                      ((None, 8, 3, lin, wrap, good, P, None, None, P), "null"),
                                      ((None, 8, 3, lin, wrap, good, P, P, None, None), "null"),
                                      ((None, 8, 0, lin, wrap, good, P, P, None, P), "1..4"),
                                      ((None, 8, 5, lin, wrap, good, P, P, None, P), "1..4"),
                                      ((None, 8, 3, 4, wrap, good, P, P, P, P), "filter"),
                                      ((None, 8, 3, -1, wrap, good, P, P, P, P), "filter"),
                                      ((None, 8, 3, lin, 2, good, P, P, P, P), "boundary"),
                                      ((None, 0, 3, lin, wrap, good, P, P, P, P), "N must"),
                                      ((None, 1 << 28, 3, mip, wrap, good, P, P, P, P), "N must"),
                                      ((None, 8, 3, mip, wrap, good, P, P, None, P), "uv_da"),
                                      ((None, 8, 3, mip, wrap, odd, P, P, P, P), "power-of-two"),
                                      ((None, 8, 3, lin, wrap, broken, P, P, P, P), "pyramid")],
        "gd_sample_texture_items": [((None, 8, 3, lin, wrap, good, None, None, P, P, P), "null"),
                                    ((None, 8, 3, lin, wrap, good, P, None, None, P, P), "null"),
                                    ((None, 8, 3, lin, wrap, good, P, None, P, None, P), "null"),
                                    ((None, 8, 3, lin, wrap, good, P, None, P, P, None), "null"),
                                    ((None, 8, 5, lin, wrap, good, P, None, P, P, P), "1..4"),
                                    ((None, 8, 3, 7, wrap, good, P, P, P, P, P), "filter"),
                                    ((None, 8, 3, lin, -1, good, P, P, P, P, P), "boundary"),
                                    ((None, 8, 3, F["linear-mipmap-nearest"], wrap, odd, P, P, P, P, P), "power-of-two"),
                                    ((None, 8, 3, mip, wrap, good, P, None, P, P, P), "uv_da")],
        "gd_sample_texture_reduce": [((None, 8, 3, good, None, P, P, P), "null"), ((None, 8, 3, good, P, P, P, None), "null"),
                                     ((None, 0, 3, good, P, P, P, P), "items"), ((None, 1 << 31, 3, good, P, P, P, P), "items"),
                                     ((None, 8, 0, good, P, P, P, P), "1..4"), ((None, 8, 3, broken, P, P, P, P), "pyramid")],
        "gd_sample_texture_fold": [((None, 3, good, None, P), "null"), ((None, 3, good, P, None), "null"),
                                   ((None, 5, good, P, P), "1..4"), ((None, 3, broken, P, P), "pyramid")],
    }


@pytest.mark.parametrize("name", ["gd_sample_rast_db", "gd_sample_interpolate_da", "gd_sample_build_mips",
                                  "gd_sample_texture_forward", "gd_sample_texture_items", "gd_sample_texture_reduce",
                                  "gd_sample_texture_fold"])
def test_bad_calls_return_minus_one_with_a_message(name):
    n = _native()
    L = n.lib()
    for i, (args, piece) in enumerate(_bad_calls()[name]):
        assert getattr(L, name)(*args) == -1, (name, i)
        text = L.gd_mesh_last_error().decode()
        assert text.startswith("sample ") and piece in text, (name, i, text)
        with pytest.raises(RuntimeError, match=name):
            n.checked(name, -1)


def test_cpu_tensors_and_unknown_modes_are_refused():
    import torch
    from garmentdreamer_amd import texture_sample as ts
    tex, uv = torch.zeros(4, 4, 3), torch.zeros(5, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ts.texture(tex, uv)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ts.build_mipmaps(tex)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ts.rast_derivatives(torch.zeros(4, 4, 4), torch.zeros(3, 4), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ts.interpolate_derivatives(torch.zeros(3, 2), torch.zeros(4, 4, 4), torch.zeros(4, 4, 4),
                                   torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="ssaa"):
        ts.render_mesh(None, None, None, None, None, None, None, None, 8, 8, ssaa=2)
    assert set(ts.MIP_FILTERS) == {"linear-mipmap-nearest", "linear-mipmap-linear"}


# ---- the statement against independent facts --------------------------------------------------------------------------

# What fp32 costs the statement: q_i = x_i - fx w_i carries an absolute error of two roundings of numbers up to 4
# (2^-22 = 2.4e-7) against a triangle extent of at least 0.02 in the same units (the tube's faces at 33 x 17): 1.2e-5 per
# factor, a few dozen operations deep.
FP32_REL = 1e-3


def _check_against_differences(pos, tri, H, W, pixels, rel):
    rast = mref.rasterize(pos, tri, H, W)
    db64 = sref.rast_db(rast, pos, tri, np.float64)
    db32 = sref.rast_db(rast, pos, tri, np.float32)
    assert db32.dtype == np.float32
    h = 1e-4
    seen = 0
    for r, c in pixels:
        t = int(rast[r, c, 3]) - 1
        if t < 0:
            assert not db64[r, c].any()
            continue
        seen += 1
        P = pos[tri[t]]
        X, Y = c + 0.5, r + 0.5
        ux = [(a - b) / (2 * h) for a, b in zip(sref.ideal_uv_at(P, X + h, Y, H, W), sref.ideal_uv_at(P, X - h, Y, H, W))]
        uy = [(a - b) / (2 * h) for a, b in zip(sref.ideal_uv_at(P, X, Y + h, H, W), sref.ideal_uv_at(P, X, Y - h, H, W))]
        want = np.array([ux[0], uy[0], ux[1], uy[1]])
        scale = np.abs(want).max()
        assert np.abs(db64[r, c] - want).max() <= 1e-6 * scale, (r, c, db64[r, c], want)     # h^2 times the third derivative
        assert np.abs(db32[r, c] - want).max() <= rel * scale, (r, c, db32[r, c], want)
    return seen, rast, db64


def test_rast_db_equals_central_differences_under_perspective():
    """the w_varies triangle of tests/mesh_scenes.py: w differs between the corners, so (u, v) is not affine in the pixel"""
    corners = np.asarray(scenes.EXTRA["w_varies"], dtype=np.float32)
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    H, W = 17, 33
    seen, rast, db = _check_against_differences(corners, tri, H, W, [(r, c) for r in range(H) for c in range(W)], FP32_REL)
    assert seen >= 3
    hit = rast[..., 3] > 0
    assert np.ptp(db[hit][:, 0]) > 1e-3 * np.abs(db[hit][:, 0]).max()            # perspective: the derivative varies
    assert not db[~hit].any()


def test_rast_db_on_the_tube_at_33x17():
    pos, tri = scenes.tube_clip()
    H, W = 17, 33
    seen, rast, db = _check_against_differences(pos, tri, H, W, [(r, c) for r in range(H) for c in range(W)], FP32_REL)
    assert seen > 50 and (rast[..., 3] == 0).any()
    # the tube flattened to w = 1, its own screen position as the attribute: the attribute derivatives reproduce the
    # pixel grid, d(x_ndc)/dX = 2 / W and d(x_ndc)/dY = 0
    ndc = (pos[:, :2] / pos[:, 3:4]).astype(np.float32)
    flat = np.concatenate((ndc, np.zeros_like(ndc[:, :1]), np.ones_like(ndc[:, :1])), axis=1).astype(np.float32)
    rast2 = mref.rasterize(flat, tri, H, W)
    da = sref.interpolate_da(ndc, rast2, sref.rast_db(rast2, flat, tri, np.float64), tri, np.float64)
    hit = rast2[..., 3] > 0
    assert hit.sum() > 50
    assert np.abs(da[hit] - np.array([2.0 / W, 0.0, 0.0, 2.0 / H])).max() < 1e-9
    assert not da[~hit].any()


def test_level_is_log2_of_the_largest_singular_value():
    rng = np.random.RandomState(3)
    Ht, Wt, L = 64, 256, 8
    J = rng.standard_normal((200, 2, 2)) * np.exp(rng.uniform(-3, 3, (200, 1, 1)))       # texels per pixel
    da = np.stack((J[:, 0, 0] / Wt, J[:, 0, 1] / Wt, J[:, 1, 0] / Ht, J[:, 1, 1] / Ht), axis=1)
    sigma = np.linalg.svd(J, compute_uv=False)[:, 0]
    want = np.clip(np.log2(sigma), 0, L)
    assert (want > 0).sum() > 20 and (want == 0).sum() > 20
    assert np.abs(sref.mip_level(da, Ht, Wt, L, np.float64) - want).max() < 1e-9
    got32 = sref.mip_level(da.astype(np.float32), Ht, Wt, L, np.float32)
    assert got32.dtype == np.float32 and np.abs(got32 - want).max() < 1e-4
    odd = np.array([[0, 0, 0, 0], [np.nan, 0, 0, 0], [np.inf, 0, 0, 1], [1e30, 0, 0, 0]], dtype=np.float32)
    assert sref.mip_level(odd, Ht, Wt, L, np.float32).tolist() == [0, 0, 0, 0]            # m <= 0 or not finite


def test_a_constant_texture_gives_a_constant_pyramid():
    for H, W in ((1, 1), (4, 8), (16, 16), (32, 64), (1, 8), (8, 1)):
        for dtype in (np.float32, np.float64):
            levels = sref.build_mips(np.full((H, W, 3), 0.3, dtype=np.float32), None, dtype)
            assert [lv.shape[:2] for lv in levels] == sref.pyramid_shapes(H, W)
            assert levels[-1].shape[:2] == (1, 1)
            for lv in levels:
                assert lv.dtype == dtype and (lv == np.float32(0.3)).all()
    with pytest.raises(ValueError):
        sref.build_mips(np.zeros((5, 7, 1), np.float32))
    assert len(sref.build_mips(np.zeros((5, 7, 1), np.float32), 0)) == 1
    assert len(sref.build_mips(np.zeros((16, 16, 1), np.float32), 1)) == 2
    ramp = np.arange(8, dtype=np.float32).reshape(2, 4, 1)
    lv = sref.build_mips(ramp)
    assert lv[1].ravel().tolist() == [2.5, 4.5] and lv[2].ravel().tolist() == [3.5]


def _mip_case(rng, Ht, Wt, N):
    L = len(sref.pyramid_shapes(Ht, Wt)) - 1
    uv = rng.uniform(-0.5, 1.5, (N, 2)).astype(np.float32)
    level = rng.uniform(-1, L + 1, N)
    s = 2.0 ** level
    da = np.stack((s / Wt, np.zeros(N), np.zeros(N), s / Ht), axis=1).astype(np.float32)
    return uv, da


@pytest.mark.parametrize("filter_name", sorted(sref.FILTERS))
@pytest.mark.parametrize("boundary_name", sorted(sref.BOUNDARIES))
def test_the_backward_statement_is_the_adjoint_of_the_forward(filter_name, boundary_name):
    """<texture(T), G> = <T, dtex(G)> in float64, for a texture T and an output gradient G drawn at random"""
    rng = np.random.RandomState(11)
    fid, bid = sref.FILTERS[filter_name], sref.BOUNDARIES[boundary_name]
    for Ht, Wt in ((1, 1), (4, 8), (16, 16)):
        T = rng.standard_normal((Ht, Wt, 3))
        uv, da = _mip_case(rng, Ht, Wt, 60)
        uv[7] = np.nan
        G = rng.standard_normal((60, 3))
        top = None if fid >= sref.LINEAR_MIPMAP_NEAREST else 0
        out = sref.texture(sref.build_mips(T, top, np.float64), uv, da, fid, bid, np.float64)
        assert not out[7].any()
        dtex = sref.texture_backward(sref.pyramid_shapes(Ht, Wt, top), uv, da, G, fid, bid, np.zeros_like(T), np.float64)
        lhs, rhs = (out * G).sum(), (T * dtex).sum()
        assert abs(lhs - rhs) <= 1e-10 * (np.abs(out * G).sum() + 1), (Ht, Wt, lhs, rhs)
        # added to what dtex holds; a texel nothing reaches keeps its value
        again = sref.texture_backward(sref.pyramid_shapes(Ht, Wt, top), uv, da, G, fid, bid, np.ones_like(T), np.float64)
        assert np.allclose(again, 1 + dtex, rtol=0, atol=1e-12)


# ---- PNG --------------------------------------------------------------------------------------------------------------

def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def _encode(img, kinds, depth=8, colour=None, interlace=0):
    """a PNG of ``img`` uint8 [H,W,3 or 4] whose row r is filtered with kinds[r % len(kinds)], by the PNG specification"""
    H, W, bpp = img.shape
    rows = img.reshape(H, W * bpp).astype(np.int64)
    raw = bytearray()
    for r in range(H):
        kind = kinds[r % len(kinds)]
        cur, up = rows[r].tolist(), (rows[r - 1].tolist() if r else [0] * (W * bpp))
        raw.append(kind)
        for i, x in enumerate(cur):
            a = cur[i - bpp] if i >= bpp else 0
            c = up[i - bpp] if i >= bpp else 0
            pred = (0, a, up[i], (a + up[i]) >> 1, _paeth(a, up[i], c), 0)[kind]       # 5: undefined, for the refusal
            raw.append((x - pred) & 255)
    colour = (2 if bpp == 3 else 6) if colour is None else colour
    body = zlib.compress(bytes(raw), 6)
    half = len(body) // 2                                                      # two IDAT chunks: the reader must join them
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, interlace))
            + _chunk(b"tEXt", b"Comment\x00made by the test") + _chunk(b"IDAT", body[:half]) + _chunk(b"IDAT", body[half:])
            + _chunk(b"IEND", b""))


@pytest.mark.parametrize("shape", ((1, 1), (5, 3), (64, 64)))
def test_png_round_trip(tmp_path, shape):
    from garmentdreamer_amd import export
    img = np.random.RandomState(shape[0]).randint(0, 256, shape + (3,)).astype(np.uint8)
    path = export.save_image_rgb(str(tmp_path / "a.png"), img)
    back = export.load_image_rgb(path)
    assert back.dtype == np.uint8 and back.shape == img.shape and np.array_equal(back, img)


def test_png_filter_types_rgba_and_refusals(tmp_path):
    from garmentdreamer_amd import export
    rng = np.random.RandomState(2)
    smooth = (np.add.outer(np.arange(9) * 7, np.arange(13) * 5)[..., None] + rng.randint(0, 40, (9, 13, 3))).astype(np.uint8)
    path = str(tmp_path / "f.png")
    for kinds in ((0,), (1,), (2,), (3,), (4,), (4, 3, 2, 1, 0)):
        with open(path, "wb") as f:
            f.write(_encode(smooth, kinds))
        assert np.array_equal(export.load_image_rgb(path), smooth), kinds
    rgba = rng.randint(0, 256, (6, 5, 4)).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(_encode(rgba, (4, 1, 3)))
    assert np.array_equal(export.load_image_rgb(path), rgba)
    export.save_image_rgba(path, rgba[..., :3] / 255.0, (rgba[..., 3] > 127).astype(np.float32))
    back = export.load_image_rgb(path)
    assert back.shape == (6, 5, 4) and np.array_equal(back[..., :3], rgba[..., :3])
    for kwargs, piece in ((dict(depth=16), "bit depth 16"), (dict(interlace=1), "interlaced"), (dict(colour=3), "colour type 3"),
                          (dict(colour=0), "colour type 0")):
        with open(path, "wb") as f:
            f.write(_encode(smooth, (0,), **kwargs))
        with pytest.raises(ValueError, match=piece):
            export.load_image_rgb(path)
    with open(path, "wb") as f:
        f.write(_encode(smooth, (5,)))
    with pytest.raises(ValueError, match="row filter type 5"):
        export.load_image_rgb(path)
    with open(path, "wb") as f:
        f.write(b"not a png at all")
    with pytest.raises(ValueError, match="signature"):
        export.load_image_rgb(path)


# ---- files ------------------------------------------------------------------------------------------------------------

def test_textured_obj_round_trip(tmp_path):
    from garmentdreamer_amd import texture_bake as tb
    from garmentdreamer_amd import texture_sample as ts
    v, tri, _ = scenes.tube(8, 3)
    vt, ft = tb.grid_atlas(tri.shape[0], 64)
    rng = np.random.RandomState(4)
    vt = np.concatenate((vt, rng.uniform(0, 1, (5, 2)).astype(np.float32)))            # values off the texel grid too
    ft = ft.copy()
    ft[0] = (vt.shape[0] - 1, vt.shape[0] - 2, vt.shape[0] - 3)
    albedo = rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    paths = tb.write_textured_obj(str(tmp_path / "m.obj"), v, tri, vt, ft, albedo)
    v2, f2, vt2, ft2, albedo2 = ts.load_textured_obj(paths[0])
    assert np.array_equal(vt2.astype(np.float32), vt) and np.array_equal(vt2, vt.astype(np.float64))
    assert np.array_equal(ft2, ft) and np.array_equal(f2, tri)
    assert np.array_equal(v2.astype(np.float32), v)
    assert albedo2.dtype == np.uint8 and np.array_equal(albedo2, albedo)
    with open(str(tmp_path / "bare.obj"), "w") as f:
        f.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    with pytest.raises(ValueError, match="texture coordinates"):
        ts.load_textured_obj(str(tmp_path / "bare.obj"))
