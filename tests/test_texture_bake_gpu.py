"""GPU checks of the texture bake (csrc/raster_bake.hip, garmentdreamer_amd/texture_bake.py) against the CPU statement of
its definition (tests/bake_reference.py): the padding index on every texel with nothing left out (integers: equality),
the 8-bit resolve against float32 numpy (one product and a truncation: equality), and the whole bake of the tube of
tests/mesh_scenes.py on a ``grid_atlas`` at 256 x 256 against the CPU rasterizer (tests/mesh_reference.py) and the
float64 field (tests/texture_reference.py).  Every raw call starts from an output buffer full of garbage."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import bake_reference as bref
from tests import mesh_reference as mref
from tests import mesh_scenes as scenes
from tests import texture_reference as tref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FUSED_KW = dict(num_levels=16, base_resolution=2, per_level_scale=1.3, log2_hashmap_size=10)   # DESIGN.md 3.20's layout
GARBAGE = 0x7F7F7F7F


def _tb():
    from garmentdreamer_amd import texture_bake
    return texture_bake


def _lib():
    from garmentdreamer_amd import _native
    return _native.lib()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _raw_pad(mask, p):
    """gd_bake_pad_index on a numpy mask into a garbage-filled ``src``; returns the tensor"""
    m = torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(DEV)
    H, W = m.shape
    src = torch.full((H, W), GARBAGE, dtype=torch.int32, device=DEV)
    ret = _lib().gd_bake_pad_index(_stream(), H, W, p, m.data_ptr(), src.data_ptr())
    assert ret == 0, _lib().gd_bake_last_error()
    return src


def _check_pad(mask, p):
    want = bref.pad_index(mask, p)
    got = _raw_pad(mask, p)
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (mask.shape, p)         # every texel, garbage overwritten
    return got, want


@pytest.mark.parametrize("case", bref.ATLAS_CASES, ids=lambda c: "res%d_n%d_g%d_p%d" % c)
def test_pad_index_atlas_masks(case):
    res, n, gutter, p = case
    mask = bref.atlas_mask(res, n, gutter)
    got, want = _check_pad(mask, p)
    assert (want >= 0).sum() > mask.sum()
    # the public form: bool mask, same answer
    assert torch.equal(_tb().uv_padding_index(torch.from_numpy(mask).to(DEV), p), got)


@pytest.mark.parametrize("p", (0, 1, 5, 64))
def test_pad_index_random_blobs_37x53(p):
    """neither side a multiple of the tile, three tiles by four"""
    mask = bref.blob_mask(37, 53, seed=7)
    got, want = _check_pad(mask, p)
    if p == 0:
        assert (want[~mask] == -1).all()
    # a nonzero byte other than 1 is covered too
    m = torch.from_numpy(mask.astype(np.uint8) * 200).to(DEV)
    assert torch.equal(_tb().uv_padding_index(m, p), got)


def test_pad_index_empty_full_corners_and_far_sources():
    own = lambda H, W: np.arange(H * W, dtype=np.int32).reshape(H, W)               # noqa: E731
    for H, W in ((1, 1), (16, 16), (33, 17)):
        got, want = _check_pad(np.zeros((H, W), dtype=bool), 7)
        assert (want == -1).all()
        got, want = _check_pad(np.ones((H, W), dtype=bool), 7)
        assert np.array_equal(want, own(H, W))
    # one covered texel in each corner, p = 3: the image border and the L1 diamond
    H, W = 21, 19
    corners = ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))
    every = np.zeros((H, W), dtype=bool)
    for r, c in corners:
        one = np.zeros((H, W), dtype=bool)
        one[r, c] = every[r, c] = True
        got, want = _check_pad(one, 3)
        assert (want >= 0).sum() == 10                     # the quarter of the diamond that is inside: 4 + 3 + 2 + 1
    _check_pad(every, 3)
    # sources several tiles away from the texels they fill, p = 64: across columns, across rows, and both
    far = np.zeros((90, 150), dtype=bool)
    far[:, 0] = True
    got, want = _check_pad(far, 64)
    assert np.array_equal(want[:, 1:65], np.broadcast_to(own(90, 150)[:, :1], (90, 64))) and (want[:, 65:] == -1).all()
    got, want = _check_pad(far.T.copy(), 64)
    assert (want[65:] == -1).all() and (want[:65] >= 0).all()
    far = np.zeros((100, 90), dtype=bool)
    far[80:83, 84:88] = True
    far[2, 3] = True
    got, want = _check_pad(far, 64)
    filled = (want >= 0) & ~far
    r, c = np.nonzero(filled)
    assert filled.sum() > 3000 and (np.abs(r - want[filled] // 90) + np.abs(c - want[filled] % 90)).max() == 64


def test_pad_index_reruns_are_identical():
    mask = bref.blob_mask(37, 53, seed=7)
    a, b = _raw_pad(mask, 64), _raw_pad(mask, 64)
    assert torch.equal(a, b)
    m = torch.from_numpy(mask).to(DEV)
    assert torch.equal(_tb().uv_padding_index(m, 5), _tb().uv_padding_index(m, 5))


def _resolve_inputs(C, H=29, W=31):
    """values just below and at every k / 255, below 0, above 1, NaN and infinities, then random; sources with -1"""
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    special = np.concatenate((k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
                              np.float32([-0.0, -1e-8, -3.5, 1.0000001, 7.0, np.nan, np.inf, -np.inf, 0.999999, 0.5])))
    rng = np.random.RandomState(C)
    flat = rng.uniform(-0.2, 1.2, size=H * W * C).astype(np.float32)
    flat[:special.size] = special
    image = rng.permutation(flat).reshape(H, W, C)
    src = rng.permutation(H * W).astype(np.int32).reshape(H, W)
    src[rng.randint(0, H, 40), rng.randint(0, W, 40)] = -1
    src[0, 0], src[0, 1] = -7, -(1 << 31)
    return image, src


@pytest.mark.parametrize("C", (1, 3, 4))
def test_resolve_u8(C):
    image, src = _resolve_inputs(C)
    want = bref.resolve_u8(image, src)
    # the reference's own arithmetic, spelt out on the boundaries: truncation, not rounding
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    assert np.array_equal(bref.resolve_u8(k.reshape(16, 16, 1), np.arange(256).reshape(16, 16))[..., 0].ravel(),
                          (k * np.float32(255.0)).astype(np.int32).astype(np.uint8))
    img, s = torch.from_numpy(image).to(DEV), torch.from_numpy(src).to(DEV)
    H, W = src.shape
    out = torch.full((H, W, C), 0x5A, dtype=torch.uint8, device=DEV)
    ret = _lib().gd_bake_resolve_u8(_stream(), H, W, C, img.data_ptr(), s.data_ptr(), out.data_ptr())
    assert ret == 0, _lib().gd_bake_last_error()
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    assert (want[src < 0] == 0).all() and want.max() == 255 and len(np.unique(want)) == 256
    assert torch.equal(_tb().resolve_u8(img, s), out)
    # uv_padding = index, then resolve
    mask = bref.blob_mask(H, W, seed=3)
    padded = _tb().uv_padding(img, torch.from_numpy(mask).to(DEV), 5)
    assert torch.equal(padded.cpu(), torch.from_numpy(bref.resolve_u8(image, bref.pad_index(mask, 5))))


RES, PAD = 256, 4


def _dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _baked():
    """the tube, a field with random parameters at the fused test layout, and its bake; shared and treated as read-only"""
    from garmentdreamer_amd import texture_field as tf
    tb = _tb()
    lay = tref.layout(**FUSED_KW)
    g = torch.Generator().manual_seed(21)
    rnd = lambda *shape, s=1.0: ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * s).float()   # noqa: E731
    p = dict(grid=rnd(int(lay["offset"][-1]) * 2), w1=rnd(32, 32, s=0.3), b1=rnd(32, s=0.3), w2=rnd(3, 32, s=0.3),
             b2=rnd(3, s=0.3))
    fld = tf.TextureField(tf.HashGridEncoder.from_layout(tf.grid_layout(16, 2, 1.3, 10))).to(DEV)
    with torch.no_grad():
        fld.encoder.params.copy_(p["grid"].to(DEV))
        for dst, k in zip(fld.mlp.parameters(), ("w1", "b1", "w2", "b2")):
            dst.copy_(p[k].to(DEV))
    v, tri, vn = scenes.tube(24, 12)
    vt, ft = tb.grid_atlas(tri.shape[0], RES)
    out = tb.bake_texture(fld, _dv(v), _dv(tri), vt, ft, resolution=RES, padding=PAD)
    return dict(lay=lay, p=p, field=fld, v=v, tri=tri, vn=vn, vt=vt, ft=ft, out=out)


def _atlas_xyz(q):
    """the positions the bake evaluates, formed again with the package's own rasterizer"""
    from garmentdreamer_amd import mesh_render as mr
    pos = np.concatenate((q["vt"] * np.float32(2) - np.float32(1), np.zeros((q["vt"].shape[0], 1), np.float32),
                          np.ones((q["vt"].shape[0], 1), np.float32)), axis=1).astype(np.float32)
    rast = mr.rasterize(_dv(pos), _dv(q["ft"]), (RES, RES))
    return pos, mr.interpolate(_dv(q["v"]), rast, _dv(q["tri"]))


def test_bake_texture_on_the_tube():
    q = _baked()
    out = q["out"]
    albedo, mask, src = out["albedo"], out["mask"], out["src"]
    assert albedo.is_cuda and albedo.dtype == torch.uint8 and tuple(albedo.shape) == (RES, RES, 3)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (RES, RES) and src.dtype == torch.int32
    pos, xyz = _atlas_xyz(q)
    # coverage: the CPU rasterizer's, and the integer restatement of its rule
    cover = mref.rasterize(pos, q["ft"], RES, RES, window=32)[..., 3] > 0
    assert np.array_equal(mask.cpu().numpy(), cover)
    assert np.array_equal(cover, bref.chart_coverage(q["vt"], q["ft"], RES, RES))
    assert 0.3 < cover.mean() < 0.9
    # covered texels: the field called directly on the same points, quantised on the host -- bit for bit
    with torch.no_grad():
        direct = q["field"](xyz.view(-1, 3), mask.view(-1)).view(RES, RES, 3).cpu().numpy()
    own = np.arange(RES * RES, dtype=np.int32).reshape(RES, RES)
    want8 = bref.resolve_u8(direct, own)
    got8 = albedo.cpu().numpy()
    assert np.array_equal(got8[cover], want8[cover])
    # ... and within one level of the float64 field: its error is ~1e-5, far below 1 / 255, so only a value on a
    # quantisation boundary can move, by one level
    p64 = {k: a.double() for k, a in q["p"].items()}
    pts = xyz.view(-1, 3).cpu()[torch.from_numpy(cover.ravel())]
    c64 = tref.field(pts, p64["grid"], p64["w1"], p64["b1"], p64["w2"], p64["b2"], q["lay"]).numpy()
    level64 = np.floor(np.clip(c64, 0, 1) * 255.0)
    diff = np.abs(got8[cover].astype(np.float64) - level64)
    print(f"covered texels {int(cover.sum())}, levels off the float64 field: {int((diff > 0).sum())} of {diff.size}, "
          f"max {diff.max():.0f}; distinct levels {len(np.unique(got8[cover]))}")
    assert diff.max() <= 1
    assert len(np.unique(got8[cover])) > 20                 # a field that varies: a wrong source would show
    # padding: every texel with a source holds that source's colour; the rest is 0; covered texels are their own source
    s = src.cpu().numpy()
    flat = got8.reshape(-1, 3)
    assert np.array_equal(s[cover], own[cover])
    assert np.array_equal(got8[s >= 0], flat[s[s >= 0]])
    assert (got8[s < 0] == 0).all() and (s < 0).any() and ((s >= 0) & ~cover).sum() > 1000
    assert torch.equal(src, _tb().uv_padding_index(mask, PAD))
    filled = np.flatnonzero((s >= 0).ravel() & ~cover.ravel())
    d1 = np.abs(filled // RES - s.ravel()[filled] // RES) + np.abs(filled % RES - s.ravel()[filled] % RES)
    assert cover.ravel()[s.ravel()[filled]].all() and 1 <= d1.min() and d1.max() <= 2 * PAD


def _check_export(tmp_path, name, **kw):
    from PIL import Image
    from garmentdreamer_amd import texture_field as tf
    tb = _tb()
    q = _baked()
    renderer = tf.NeTFRenderer(_dv(q["v"]), _dv(q["tri"]), _dv(q["vn"]), q["field"])
    path = str(tmp_path / name / "final_mesh_finetuned.obj")
    written = renderer.export_mesh(path, texture_resolution=RES, padding=PAD, **kw)
    stem = os.path.splitext(path)[0]
    assert written == [path, stem + ".mtl", stem + "_albedo.png"] and all(os.path.isfile(p) for p in written)
    v2, f2, vt2, ft2 = tb.load_obj_uv(path)
    F = q["tri"].shape[0]
    assert f2.shape == (F, 3) and ft2.shape == (F, 3) and np.array_equal(f2, q["tri"].astype(np.int64))
    want_v = q["v"].astype(np.float64) * (np.array([-1.0, 1.0, 1.0]) if kw.get("reverse") else 1.0)
    assert np.array_equal(v2, want_v)
    return np.asarray(Image.open(written[2])), vt2, ft2


def test_export_mesh_writes_the_three_files(tmp_path):
    q = _baked()
    png, vt2, ft2 = _check_export(tmp_path, "own_atlas", reverse=True)
    assert np.array_equal(png, q["out"]["albedo"].cpu().numpy())
    assert np.array_equal(ft2, q["ft"].astype(np.int64))
    assert np.array_equal(vt2[:, 0], q["vt"][:, 0].astype(np.float64))
    assert np.array_equal(vt2[:, 1], 1.0 - q["vt"][:, 1].astype(np.float64))


def test_export_mesh_with_the_callers_uvs(tmp_path):
    """another atlas of the same mesh (a wider gutter), its faces in another order of corners"""
    tb = _tb()
    q = _baked()
    vt, ft = tb.grid_atlas(q["tri"].shape[0], RES, gutter=2)
    perm = np.random.RandomState(0).permutation(vt.shape[0])
    vt_mine = vt[perm]
    ft_mine = np.argsort(perm).astype(np.int32)[ft]          # the same triangles through shuffled coordinates
    png, vt2, ft2 = _check_export(tmp_path, "callers", vt=vt_mine, ft=torch.from_numpy(ft_mine))
    want = tb.bake_texture(q["field"], _dv(q["v"]), _dv(q["tri"]), vt, ft, resolution=RES, padding=PAD)
    assert np.array_equal(png, want["albedo"].cpu().numpy())
    assert not np.array_equal(png, q["out"]["albedo"].cpu().numpy())
    assert np.array_equal(ft2, ft_mine.astype(np.int64)) and vt2.shape == (vt.shape[0], 2)
