"""GPU checks of reading the captured views (garmentdreamer_amd/views.py, the entries of include/gd_views.h in
csrc/raster_views.hip): the unfilter bit for bit against the pixels the test encoder was given, the unpack bit for bit
against the torch statement, ``read_views`` / ``read_fit_views`` on a written capture, and the deformer fed from views."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import remesh_reference as rr
from tests import views_reference as vref

pytestmark = pytest.mark.gpu
DEV = "cuda"

# the first row and the first pixel without neighbours, one row past a 64-row band, two bands and a tail, widths that are
# no multiple of the 64-pixel chunk and one past two chunks
SHAPES = [(1, 1, 4), (1, 7, 3), (5, 1, 4), (3, 2, 3), (64, 64, 4), (65, 33, 4), (130, 67, 3), (257, 129, 4)]
MODES = [0, 1, 2, 3, 4, "mixed"]
BATCH = 3


@functools.lru_cache(maxsize=None)
def _batch(shape, mode, content):
    """(filtered uint8 [B, H (1 + W bpp)], pixels uint8 [B,H,W,bpp]): other content and another filter map per image: a
    seeded random type per row, or every row of type ``mode`` in image 0, ``mode + 1`` in image 1, ... (mod 5)"""
    H, W, bpp = shape
    pixels = [vref.random_pixels(H, W, bpp, 7 * b + 1) if content == "random" else np.roll(vref.ramp_pixels(H, W, bpp), b, axis=1)
              for b in range(BATCH)]
    kinds = [vref.kinds_for(H, "mixed", seed=b + 3) if mode == "mixed" else vref.kinds_for(H, (mode + b) % 5)
             for b in range(BATCH)]
    return np.stack([vref.filter_rows(p, k) for p, k in zip(pixels, kinds)]).reshape(BATCH, -1), np.stack(pixels)


@pytest.mark.parametrize("content", ["random", "ramp"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unfilter_is_exact(shape, mode, content):
    from garmentdreamer_amd import views
    H, W, bpp = shape
    filtered, pixels = _batch(shape, mode, content)
    if mode != "mixed":
        assert (filtered.reshape(BATCH, H, -1)[0, :, 0] == mode).all()
    f = torch.from_numpy(filtered).to(DEV)
    out = views.png_unfilter(f, BATCH, H, W, bpp)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (BATCH, H, W, bpp)
    assert torch.equal(out.cpu(), torch.from_numpy(pixels))
    assert torch.equal(views.png_unfilter(f, BATCH, H, W, bpp), out)      # a second launch
    one = views.png_unfilter(f.reshape(BATCH, -1)[1].clone(), 1, H, W, bpp)   # the streams are independent
    assert torch.equal(one[0], out[1])


def test_unfilter_treats_an_undefined_type_as_none_and_ends():
    """the host refuses such a stream; the device must still end on it, whatever it holds"""
    from garmentdreamer_amd import views
    rng = np.random.default_rng(0)
    rows = rng.integers(0, 256, size=(70, 1 + 9 * 4), dtype=np.uint8)     # random types, most of them undefined
    out = views.png_unfilter(torch.from_numpy(rows).to(DEV).reshape(-1), 1, 70, 9, 4)
    assert np.array_equal(out.cpu().numpy().reshape(70, -1), vref.unfilter(rows, 4))


# ---- the unpack ------------------------------------------------------------------------------------------------------

def _bits(t):
    return t.contiguous().view(torch.int32)


def test_unpack_every_byte_value():
    from garmentdreamer_amd import views
    pins = np.load(os.path.join(os.path.dirname(__file__), "golden", "views_pins.npz"))
    normal_rgba, rgba = vref.every_byte_image(10), vref.every_byte_image(20)
    assert np.array_equal(normal_rgba, pins["image/normal_rgba"]) and np.array_equal(rgba, pins["image/rgba"])
    for c in range(4):
        assert sorted(normal_rgba[..., c].reshape(-1).tolist()) == list(range(256))
    want = vref.unpack_torch(normal_rgba, rgba)
    for channels in (4, 3):
        got = views.unpack_view(torch.from_numpy(normal_rgba).to(DEV), torch.from_numpy(rgba[..., :channels].copy()).to(DEV))
        for g, w, name in zip(got, want, ("normal", "mask", "rgb")):
            assert g.dtype == torch.float32 and g.shape == w.shape, name
            assert torch.equal(_bits(g.cpu()), _bits(w)), name
            assert np.array_equal(g.cpu().numpy(), pins["image/" + name]), name      # what the reference's View.load made
    for g, w in zip(got, vref.unpack(normal_rgba, rgba)):                 # the numpy statement says the same
        assert np.array_equal(g.cpu().numpy().view(np.int32), w.view(np.int32))
    rgb, mask = views.unpack_rgba(torch.from_numpy(rgba).to(DEV))
    assert torch.equal(_bits(rgb.cpu()), _bits(want[2])) and np.array_equal(mask.cpu().numpy(), pins["image/mask4"])
    assert np.array_equal(rgb.cpu().numpy(), pins["image/rgb4"])
    # a pixel count that is no multiple of four, from a tensor that does not start on 16 bytes
    odd = torch.from_numpy(np.concatenate((np.zeros(4, np.uint8), normal_rgba[:3, :5].reshape(-1)))).to(DEV)[4:].reshape(3, 5, 4)
    got = views.unpack_view(odd, odd)
    for g, w in zip(got, vref.unpack_torch(normal_rgba[:3, :5], normal_rgba[:3, :5])):
        assert torch.equal(_bits(g.cpu()), _bits(w))


# ---- a capture on disk -----------------------------------------------------------------------------------------------

def _look_at(position):
    """float32 [4,4] camera-to-world with columns (right, down, forward), looking at the origin"""
    position = np.asarray(position, dtype=np.float64)
    forward = -position / np.linalg.norm(position)
    right = np.cross(forward, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(forward, right), forward, position
    return c2w.astype(np.float32)


def _write_capture(folder, H, W, positions, fovy=0.7):
    """a capture of len(positions) views in the layout of export.dump_test_view: the records of camera_info_entry; the last
    colour image by export.save_image_rgba, every other file by the test encoder with random row types; the masks are
    discs.  Returns the byte images (normal_rgba, rgba) per view."""
    from garmentdreamer_amd import export
    records = [export.camera_info_entry(_look_at(p), i, W, H, fovy) for i, p in enumerate(positions)]
    export.save_cameras_json(os.path.join(folder, "cameras.json"), records)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    disc = ((yy - H / 2 + 0.5) ** 2 + (xx - W / 2 + 0.5) ** 2 <= (0.3 * min(H, W)) ** 2)
    for sub in ("estimated_normals", "gs_rendered_rgba"):
        os.makedirs(os.path.join(folder, sub), exist_ok=True)
    images = []
    for i in range(len(positions)):
        normal_rgba, rgba = vref.random_pixels(H, W, 4, 30 + i), vref.random_pixels(H, W, 4, 40 + i)
        normal_rgba[..., 3] = rgba[..., 3] = disc * 255
        vref.write_png(os.path.join(folder, "estimated_normals", f"{i}.png"), normal_rgba, vref.kinds_for(H, "mixed", i))
        path = os.path.join(folder, "gs_rendered_rgba", f"{i}.png")
        if i == len(positions) - 1:
            export.save_image_rgba(path, rgba[..., :3].astype(np.float32) / 255, disc.astype(np.float32))
        else:
            vref.write_png(path, rgba, vref.kinds_for(H, "mixed", 9 + i))
        images.append((normal_rgba, rgba))
    return records, images


POSITIONS = [(2.2, 0.3, 0.4), (-0.5, 2.1, 0.9), (-1.4, -1.6, -0.6)]


def test_read_views(tmp_path):
    from garmentdreamer_amd import export, views
    H, W = 20, 24
    records, images = _write_capture(str(tmp_path), H, W, POSITIONS)
    timings = {}
    got = views.read_views(str(tmp_path), timings=timings)
    assert len(got) == 3 and sorted(timings) == ["inflate", "unfilter", "unpack", "upload"]
    for i, view in enumerate(got):
        normal_rgba = export.load_image_rgb(str(tmp_path / "estimated_normals" / f"{i}.png"))
        rgba = export.load_image_rgb(str(tmp_path / "gs_rendered_rgba" / f"{i}.png"))
        assert np.array_equal(normal_rgba, images[i][0]) and np.array_equal(rgba, images[i][1])
        for g, w in zip((view.normal, view.mask, view.rgb), vref.unpack_torch(normal_rgba, rgba)):
            assert g.is_cuda and torch.equal(_bits(g.cpu()), _bits(w))
        K, R, t = views.camera_from_record(records[i])
        assert view.resolution == (H, W) and view.name == str(i)
        assert np.array_equal(view.K.numpy(), K.astype(np.float32)) and np.array_equal(view.R.numpy(), R.astype(np.float32))
        assert np.array_equal(view.t.numpy(), t.astype(np.float32)) and view.K.dtype == torch.float32
        # the camera looks at the origin: it lands on the principal point, in front
        assert torch.allclose(view.project(torch.zeros(1, 3))[0], torch.tensor([W / 2, H / 2, np.linalg.norm(POSITIONS[i])],
                                                                                dtype=torch.float32), atol=1e-3)
    # only the views asked for are opened, and they come in the order asked for
    open(tmp_path / "estimated_normals" / "1.png", "wb").write(b"garbage")
    with pytest.raises(ValueError, match=r"1\.png: not a PNG file"):
        views.read_views(str(tmp_path))
    some = views.read_views(str(tmp_path), indices=[2, 0])
    assert [v.name for v in some] == ["2", "0"]
    for v, w in zip(some, (got[2], got[0])):
        assert torch.equal(v.normal, w.normal) and torch.equal(v.mask, w.mask) and torch.equal(v.rgb, w.rgb)
    fit = views.read_fit_views(str(tmp_path))
    for i, fv in enumerate(fit):
        c2w, K = views.c2w_from_record(records[i])
        assert np.array_equal(fv.c2w, c2w.astype(np.float32)) and np.array_equal(fv.K, K.astype(np.float32))
        assert torch.equal(fv.rgb, got[i].rgb) and tuple(fv.mask.shape) == (H, W, 1)
        assert np.array_equal(fv.mask.cpu().numpy()[..., 0], images[i][1][..., 3].astype(np.float32) / np.float32(255))
    batch = views.decode_png_batch([str(tmp_path / "gs_rendered_rgba" / f"{i}.png") for i in (2, 0, 1)])
    assert tuple(batch.shape) == (3, H, W, 4) and np.array_equal(batch.cpu().numpy(), np.stack([images[i][1] for i in (2, 0, 1)]))
    vref.write_png(tmp_path / "small.png", vref.random_pixels(4, 4, 4, 0), [0] * 4)
    with pytest.raises(ValueError, match="small.png.*a batch has one geometry"):
        views.decode_png_batch([str(tmp_path / "gs_rendered_rgba" / "0.png"), str(tmp_path / "small.png")])


# ---- the deformer from views ---------------------------------------------------------------------------------------------

def _sphere():
    # closed, 128 faces: the smallest closed mesh the remesh tests use (tests/mesh_scenes.py has the open tube only)
    v, tri = rr.mesh("sphere")
    return (0.45 * v).astype(np.float32), tri.astype(np.int32)


def test_deformer_from_views_is_the_deformer_built_by_hand(tmp_path):
    from garmentdreamer_amd import texture_field as tf, views
    from garmentdreamer_amd.deformer import Deformer
    from garmentdreamer_amd.mesh_deform import GBufferRenderer
    _write_capture(str(tmp_path), 32, 32, POSITIONS)
    got = views.read_views(str(tmp_path))
    v, tri = _sphere()
    v_d, tri_d = torch.from_numpy(v).to(DEV), torch.from_numpy(tri).to(DEV)
    near, far = views.near_far(got, views.AABB(v).corners)
    assert 0 < near < far
    mine = Deformer.from_views(v_d, tri_d, got, near, far, lr=2e-3)
    mvps = [GBufferRenderer.to_gl_camera(w.K, w.R, w.t, (32, 32), n=near, f=far).to(DEV) for w in got]
    hand = Deformer(v_d, tri_d, mvps, [w.mask for w in got], [(32, 32)] * 3, lr=2e-3)
    a, b = mine.step([0, 1, 2]), hand.step([0, 1, 2])
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert float(a["mask"]) > 0 and torch.isfinite(a["total"])           # the sphere is in the picture
    mine.begin_second_stage_from_views(got)
    hand.begin_second_stage([w.normal for w in got], [w.R.to(DEV) for w in got], [w.center.to(DEV) for w in got])
    a, b = mine.step_second([2, 0]), hand.step_second([2, 0])
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(mine.offsets.detach(), hand.offsets.detach()) and mine.offsets.detach().abs().max() > 0
    # stage 4 from the same directory
    vn = torch.nn.functional.normalize(v_d, dim=1)
    field = tf.TextureField(tf.HashGridEncoder.from_layout(tf.grid_layout(16, 2, 1.3, 10),
                                                           generator=torch.Generator().manual_seed(1))).to(DEV)
    renderer = tf.NeTFRenderer(v_d, tri_d, vn, field)
    from garmentdreamer_amd.texture_fit import fit_texture
    history = fit_texture(renderer, views.read_fit_views(str(tmp_path)), iters=1, resolution=32)
    assert tuple(history.shape) == (1,) and torch.isfinite(history).all()


def test_run_deformation(tmp_path):
    from garmentdreamer_amd import deformer as dm, mesh_simplify as ms, template
    _write_capture(str(tmp_path), 32, 32, POSITIONS)
    v, tri = _sphere()
    # run_deformation maps (x, y, z) -> (z, x, y) bound: the template is written so that the sphere comes out as it is
    ms.write_obj(str(tmp_path / "template.obj"), np.stack([v[:, 1], v[:, 2], v[:, 0]], axis=1) * 2, tri)
    config = {"iterations_first": 2, "iterations_second": 2, "upsample_iterations": [4], "picked_views_first": [0, 2],
              "picked_views_second": [1, 2], "weight_shading": 0.0, "final_faces": 100}
    paths = dm.run_deformation(str(tmp_path), str(tmp_path / "template.obj"), 0.5, config)
    assert sorted(paths) == ["bbox", "final_mesh", "mesh"] and all(os.path.isfile(p) for p in paths.values())
    assert paths["final_mesh"] == str(tmp_path / "final_mesh.obj")
    assert np.allclose(np.loadtxt(paths["bbox"]), [v.min(axis=0), v.max(axis=0)], atol=1e-6)
    mv, mf = template.load_obj(paths["mesh"])
    assert np.isfinite(mv).all() and mf.shape[0] != tri.shape[0] and mv.shape[0] != v.shape[0]      # the upsample happened
    assert mf.max() == mv.shape[0] - 1 and np.abs(mv).max() < 0.9         # denormalised: the normalised box reaches 1
    fv, ff = template.load_obj(paths["final_mesh"])
    assert np.isfinite(fv).all() and 0 < ff.shape[0] <= 100 and ff.max() < fv.shape[0]
    with pytest.raises(ValueError, match="unknown config keys"):
        dm.run_deformation(str(tmp_path), str(tmp_path / "template.obj"), 0.5, {"iterations": 1})
