"""CPU-side checks of the texture bake (include/gd_bake.h, garmentdreamer_amd/texture_bake.py): the two statements of the
padding definition (tests/bake_reference.py) agree; the statement against the scipy / scikit-learn formulation that
kiui's ``uv_padding`` is understood to be; ``grid_atlas``; the files of ``write_textured_obj`` read back with
``load_obj_uv`` and Pillow; the header's entries are exported, bound and validate their arguments without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import bake_reference as bref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tb():
    from garmentdreamer_amd import texture_bake
    return texture_bake


def test_statement_forms_agree():
    """plain loops over all covered texels against the vectorised form, every texel"""
    cases = [(bref.blob_mask(20, 23, seed), p) for seed in (1, 2) for p in (0, 1, 3, 7, 64)]
    corner = np.zeros((9, 11), dtype=bool)
    corner[0, 0] = corner[8, 10] = True
    cases += [(corner, 3), (np.zeros((5, 7), dtype=bool), 4), (np.ones((5, 7), dtype=bool), 4),
              (bref.atlas_mask(48, 3, 1)[:24, :24], 2)]
    for mask, p in cases:
        loops, vec = bref.pad_index_loops(mask, p), bref.pad_index(mask, p)
        assert loops.dtype == np.int32 and np.array_equal(loops, vec), p
        own = np.arange(mask.size, dtype=np.int32).reshape(mask.shape)
        assert np.array_equal(vec[mask], own[mask])
        if p == 0:
            assert (vec[~mask] == -1).all()
    # the tie rule: two covered texels at the same distance, the lower row-major index wins
    m = np.zeros((3, 5), dtype=bool)
    m[1, 0] = m[1, 4] = True
    assert bref.pad_index(m, 4)[1, 2] == 1 * 5 + 0
    m = np.zeros((5, 3), dtype=bool)
    m[0, 1] = m[4, 1] = m[2, 0] = True                    # (2,1): distance 1 to (2,0), 2 to the others
    assert bref.pad_index(m, 4)[2, 1] == 2 * 3 + 0
    m[2, 0] = False
    m[2, 2] = False
    assert bref.pad_index(m, 4)[2, 1] == 0 * 3 + 1
    # the L1 gate: a covered texel at (3, 3) from the corner is inside the Euclidean radius 5 but outside the diamond 5
    m = np.zeros((8, 8), dtype=bool)
    m[3, 3] = True
    assert bref.pad_index(m, 5)[0, 0] == -1 and bref.pad_index(m, 6)[0, 0] == 3 * 8 + 3


@pytest.mark.parametrize("case", bref.ATLAS_CASES, ids=lambda c: "res%d_n%d_g%d_p%d" % c)
def test_statement_against_the_knn_formulation(case):
    """Same filled region, and the same colour on every filled texel whose nearest covered texel is unique (a random
    image: a wrong source shows).  Texels with more than one nearest are where the KD-tree's pick is unspecified; they
    must be at most 40 % of the filled texels, so that the comparison keeps its meaning."""
    res, n, gutter, p = case
    mask = bref.atlas_mask(res, n, gutter)
    assert mask.any() and not mask.all()
    src, ties = bref.pad_index(mask, p, with_ties=True)
    image = np.random.RandomState(res).rand(res, res, 3).astype(np.float32)
    region, padded = bref.knn_formulation(image, mask, p)
    filled = (src >= 0) & ~mask
    assert np.array_equal(region, filled)
    assert filled.sum() > 0
    share = ties.sum() / filled.sum()
    unique = filled & ~ties
    ours = image.reshape(-1, 3)[np.maximum(src, 0).ravel()].reshape(res, res, 3)
    wrong = int((ours[unique] != padded[unique]).any(axis=1).sum())
    print(f"{case}: filled {int(filled.sum())}, tied {100 * share:.1f} %, mismatches off the ties {wrong}")
    assert share <= 0.40
    assert wrong == 0
    assert np.array_equal(padded[mask], image[mask]) and np.array_equal(padded[~mask & ~region], image[~mask & ~region])


def _chart_sets(vt, ft, res):
    """per triangle the set of texel centres inside or on it (inclusive: the strictest test of disjointness)"""
    out = []
    c = np.arange(res) + 0.5
    px, py = np.meshgrid(c, c)
    for tri in ft:
        (x0, y0), (x1, y1), (x2, y2) = np.rint(vt[tri].astype(np.float64) * res)   # the corners are whole texels
        e0 = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)
        e1 = (x2 - x1) * (py - y1) - (y2 - y1) * (px - x1)
        e2 = (x0 - x2) * (py - y2) - (y0 - y2) * (px - x2)
        inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        out.append(set(np.flatnonzero(inside.ravel()).tolist()))
    return out


@pytest.mark.parametrize("F,res,gutter", [(72, 96, 1), (32, 64, 2), (18, 48, 1), (7, 40, 1), (1, 16, 2), (5, 33, 3)])
def test_grid_atlas(F, res, gutter):
    tb = _tb()
    vt, ft = tb.grid_atlas(F, res, gutter)
    assert vt.dtype == np.float32 and vt.shape == (3 * F, 2) and ft.dtype == np.int32
    assert np.array_equal(ft, np.arange(3 * F).reshape(F, 3))
    assert vt.min() >= 0.0 and vt.max() <= 1.0
    vt2, ft2 = tb.grid_atlas(F, res, gutter)
    assert np.array_equal(vt, vt2) and np.array_equal(ft, ft2)                 # deterministic
    n = int(np.ceil(np.sqrt(np.ceil(F / 2))))
    s = res // n
    leg = s - 3 * gutter
    texel = vt.astype(np.float64).reshape(F, 3, 2) * res
    assert np.abs(texel - np.rint(texel)).max() < 1e-4                         # corners on texel corners
    texel = np.rint(texel).astype(np.int64)
    for t in range(F):
        k = t // 2
        cx, cy = s * (k % n), s * (k // n)
        if t % 2 == 0:
            want = [(cx + gutter, cy + gutter), (cx + gutter + leg, cy + gutter), (cx + gutter, cy + gutter + leg)]
        else:
            a, b = cx + s - gutter, cy + s - gutter
            want = [(a, b), (a - leg, b), (a, b - leg)]
        assert texel[t].tolist() == [list(w) for w in want], t
    sets = _chart_sets(vt, ft, res)
    assert all(len(a) > 0 for a in sets)                                       # every chart owns a texel centre
    seen = set()
    for a in sets:
        assert not (a & seen)                                                  # pairwise disjoint
        seen |= a
    covered = set(np.flatnonzero(bref.chart_coverage(vt, ft, res, res).ravel()).tolist())
    assert covered <= seen and len(seen) - len(covered) <= F * leg             # they differ on hypotenuse centres only
    # the same orientation for both triangles of a cell
    e1, e2 = texel[:, 1] - texel[:, 0], texel[:, 2] - texel[:, 0]
    assert ((e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]) == leg * leg).all()


def test_grid_atlas_refuses_cells_that_are_too_small():
    tb = _tb()
    tb.grid_atlas(2, 4, 1)                                  # s = 4, leg 1: the smallest that works
    for F, res, gutter in ((2, 3, 1), (72, 17, 1), (32, 23, 2), (3, 8, 2), (0, 16, 1), (4, 0, 1)):
        with pytest.raises(ValueError):
            tb.grid_atlas(F, res, gutter)


def _toy_mesh():
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.25], [1.0, 1.0, 0.5], [-0.5, 1.0, 0.125]])
    f = np.array([[0, 1, 2], [0, 2, 3]])
    return v, f


@pytest.mark.parametrize("reverse", (False, True))
def test_write_textured_obj_round_trip(tmp_path, reverse):
    from PIL import Image
    tb = _tb()
    v, f = _toy_mesh()
    vt, ft = tb.grid_atlas(2, 16, 1)
    albedo = np.random.RandomState(4).randint(0, 256, size=(16, 16, 3)).astype(np.uint8)
    path = str(tmp_path / "sub" / "final_mesh.obj")
    written = tb.write_textured_obj(path, torch.from_numpy(v), f, vt, torch.from_numpy(ft), torch.from_numpy(albedo),
                                    reverse=reverse)
    assert written == [path, str(tmp_path / "sub" / "final_mesh.mtl"), str(tmp_path / "sub" / "final_mesh_albedo.png")]
    assert all(os.path.isfile(p) for p in written)
    text = open(path).read().splitlines()
    assert text[0] == "mtllib final_mesh.mtl" and "usemtl defaultMat" in text
    assert text.index("usemtl defaultMat") < min(i for i, l in enumerate(text) if l.startswith("f "))
    mtl = open(written[1]).read()
    assert "newmtl defaultMat" in mtl and "map_Kd final_mesh_albedo.png" in mtl.splitlines()
    v2, f2, vt2, ft2 = tb.load_obj_uv(path)
    want_v = v * np.array([-1.0, 1.0, 1.0]) if reverse else v
    assert np.array_equal(v2, want_v) and np.array_equal(f2, f)               # the faces are left alone
    assert np.array_equal(ft2, ft.astype(np.int64))
    want_vt = np.stack((vt[:, 0].astype(np.float64), 1.0 - vt[:, 1].astype(np.float64)), axis=1)
    assert np.array_equal(vt2, want_vt)                                       # v is flipped, u is not
    from garmentdreamer_amd import template
    v3, f3 = template.load_obj(path)
    assert np.array_equal(v3, v2) and np.array_equal(f3, f2)
    img = Image.open(written[2])
    assert img.mode == "RGB" and img.size == (16, 16)
    assert np.array_equal(np.asarray(img), albedo)                            # PNG row 0 is atlas row 0


def test_save_image_rgb_rejects_other_layouts(tmp_path):
    from garmentdreamer_amd import export
    for bad in (np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.uint8)):
        with pytest.raises(ValueError):
            export.save_image_rgb(str(tmp_path / "x.png"), bad)
    from PIL import Image
    wide = np.random.RandomState(0).randint(0, 256, size=(3, 7, 3)).astype(np.uint8)      # H != W
    assert np.array_equal(np.asarray(Image.open(export.save_image_rgb(str(tmp_path / "w.png"), wide))), wide)


def test_load_obj_uv(tmp_path):
    tb = _tb()
    p = tmp_path / "quad.obj"
    p.write_text("# a quad, a fan of two\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1 0\nvt 0 1\n"
                 "vn 0 0 1\nf 1/1/1 2/2/1 3/3/1 4/4/1\nf -4/-4 -3/-3 -1/-1\n")
    v, f, vt, ft = tb.load_obj_uv(str(p))
    assert v.shape == (4, 3) and f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 3]]
    assert ft.tolist() == f.tolist() and vt.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]]
    for corner in ("3", "3//1"):                            # one corner without a texture index: no UVs at all
        p.write_text(f"v 0 0 0\nv 1 0 0\nv 1 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nf 1/1 2/2 3/3\nf 1/1 2/2 {corner}\n")
        v, f, vt, ft = tb.load_obj_uv(str(p))
        assert vt is None and ft is None and f.tolist() == [[0, 1, 2], [0, 1, 2]]
    for body in ("v 0 0 0\nv 1 0 0\nv 1 1 0\nvt 0 0\nf 1/1 2/1 3/2\n",          # texture index out of range
                 "v 0 0 0\nv 1 0 0\nv 1 1 0\nvt 0 0\nf 1/0 2/1 3/1\n",          # index 0
                 "v 0 0 0\nv 1 0 0\nv 1 1 0\nvt 0 0\nf 1/-2 2/1 3/1\n",         # relative index out of range
                 "v 0 0 0\nvt 0 0\n"):                                         # no faces
        p.write_text(body)
        with pytest.raises(ValueError):
            tb.load_obj_uv(str(p))


def test_bake_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gd_bake.h")).read()
    assert "GD_BAKE_MAX_PADDING 64" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gd_bake_[a-z0-9_]+)\s*\(", text)))
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert declared == ["gd_bake_last_error", "gd_bake_pad_index", "gd_bake_resolve_u8"]
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_bake.h but not exported"
    assert sorted(_native.BAKE_SIGNATURES) == declared
    others = set(_native.SIGNATURES) | set(_native.SCENE_SIGNATURES) | set(_native.MESH_SIGNATURES) \
        | set(_native.MESH_DEFORM_SIGNATURES) | set(_native.MESH_GEOMETRY_SIGNATURES) | set(_native.TEXTURE_SIGNATURES)
    assert not set(declared) & others
    assert _native.BAKE_MAX_PADDING == 64 and _native.BAKE_MAX_CHANNELS == 4


def test_entries_validate_their_arguments():
    """-1 and a message before any device work (no GPU is touched: the stream is never used, no pointer is followed)"""
    from garmentdreamer_amd import _native
    L = _native.lib()
    err = L.gd_bake_last_error
    x = 0x1000                                              # a non-null pointer that is never followed
    pad = lambda H, W, p, mask=x, src=x: L.gd_bake_pad_index(None, H, W, p, mask, src)            # noqa: E731
    res = lambda H, W, C, im=x, src=x, out=x: L.gd_bake_resolve_u8(None, H, W, C, im, src, out)   # noqa: E731
    assert pad(8, 8, 4, mask=None) == -1 and b"pad index" in err() and b"null" in err()
    assert pad(8, 8, 4, src=None) == -1 and b"null" in err()
    for hole in ("im", "src", "out"):
        assert res(8, 8, 3, **{hole: None}) == -1 and b"resolve u8" in err() and b"null" in err(), hole
    for H, W in ((0, 8), (8, 0), (-1, 8), (8, -5), (1 << 16, 1 << 15), (1 << 30, 2), ((1 << 31) - 1, (1 << 31) - 1)):
        assert pad(H, W, 4) == -1 and b"pad index" in err() and (b"H" in err() and b"W" in err()), (H, W)
        assert res(H, W, 3) == -1 and b"resolve u8" in err() and (b"H" in err() and b"W" in err()), (H, W)
    for p in (-1, 65, 1 << 20):
        assert pad(8, 8, p) == -1 and b"padding" in err(), p
    for C in (0, 5, -3):
        assert res(8, 8, C) == -1 and b"C must" in err(), C


def test_documented_errors():
    tb = _tb()
    with pytest.raises(RuntimeError, match="no CPU path"):
        tb.uv_padding_index(torch.zeros(4, 4, dtype=torch.bool), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tb.uv_padding(torch.zeros(4, 4, 3), torch.zeros(4, 4, dtype=torch.bool), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tb.resolve_u8(torch.zeros(4, 4, 3), torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        tb.bake_texture(lambda x, m: x, torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), np.zeros((3, 2)),
                        np.zeros((1, 3)), 16, 2)
    from garmentdreamer_amd import texture_field as tf
    assert callable(tf.NeTFRenderer.export_mesh)
