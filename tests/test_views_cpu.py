"""What of reading the captured views needs no GPU (garmentdreamer_amd/views.py, include/gd_views.h): the test encoder
against the package's own PNG reader, the cameras, the box, the space normalisation, near / far and the sampler against
vectors made by the reference's code (tests/golden/views_pins.npz), the refusals, and the C-ABI."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import views_reference as vref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "views_pins.npz")


@pytest.fixture(scope="module")
def pins():
    return dict(np.load(GOLDEN))


def _records(pins):
    return json.loads(pins["records_json"].tobytes().decode())


# ---- 1. the encoder --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bpp", [3, 4])
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, "mixed"])
def test_encoder_round_trip(tmp_path, bpp, mode):
    from garmentdreamer_amd.export import load_image_rgb
    for pixels in (vref.random_pixels(9, 7, bpp, 3), vref.ramp_pixels(9, 7, bpp)):
        kinds = vref.kinds_for(9, mode, seed=5)
        rows = vref.filter_rows(pixels, kinds)
        assert rows[:, 0].tolist() == kinds.tolist()
        path = vref.write_png(tmp_path / "image.png", pixels, kinds)
        assert np.array_equal(load_image_rgb(path), pixels)
        assert np.array_equal(vref.unfilter(rows, bpp).reshape(pixels.shape), pixels)


def test_unfilter_treats_an_undefined_type_as_none():
    rows = vref.filter_rows(vref.random_pixels(3, 4, 3, 1), [0, 0, 0])
    rows[1, 0] = 9
    assert np.array_equal(vref.unfilter(rows, 3), rows[:, 1:])


# ---- 2. cameras ------------------------------------------------------------------------------------------------------

def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.finfo(np.float32).tiny)


def test_cameras_against_the_reference(pins):
    from garmentdreamer_amd import views
    records = _records(pins)
    assert len(records) >= 3
    off_axis = 0
    for i, record in enumerate(records):
        K, R, t = views.camera_from_record(record)
        assert K.dtype == R.dtype == t.dtype == np.float64
        for mine, name in ((K, "K"), (R, "R"), (t, "t")):
            assert _ulps(mine.astype(np.float32), pins[f"view{i}/{name}"]).max() <= 1, (i, name)
        off_axis += bool((np.abs(R) > 0.05).all())
        # rigid, and MIRRORED: the last flip of View.load (column 2, after column 1 was rebuilt right-handed) leaves det -1
        assert abs(np.linalg.det(R) + 1) < 1e-6 and np.allclose(R @ R.T, np.eye(3), atol=1e-6)
        c2w, K4 = views.c2w_from_record(record)
        assert np.array_equal(c2w, pins[f"view{i}/c2w"]) and np.array_equal(K4, pins[f"view{i}/K4"])
        assert K4[0, 2] == record["width"] / 2 and K4[1, 2] == record["height"] / 2
    assert off_axis >= 1


# ---- 3. the box and the space ------------------------------------------------------------------------------------------

def test_aabb_against_the_reference(pins, tmp_path):
    from garmentdreamer_amd import views
    aabb = views.AABB(pins["aabb/points"])
    assert np.array_equal(aabb.corners, pins["aabb/corners"]) and aabb.corners.dtype == pins["aabb/corners"].dtype
    assert np.array_equal(aabb.center, pins["aabb/center"]) and aabb.longest_extent == pins["aabb/longest_extent"]
    for side in (1, 2):
        A, A_inv = views.normalize_aabb(aabb, side_length=side)
        assert np.array_equal(A, pins[f"aabb/A{side}"]) and A.dtype == np.float32
        assert np.allclose(A_inv, pins[f"aabb/A{side}_inv"], rtol=1e-6, atol=0)          # np.linalg.inv: LAPACK's last bit
    assert np.array_equal(views.AABB(torch.from_numpy(pins["aabb/points"])).corners, aabb.corners)
    aabb.save(tmp_path / "bbox.txt")
    again = views.AABB.load(tmp_path / "bbox.txt")
    assert np.array_equal(again.min_p, aabb.min_p) and np.array_equal(again.max_p, aabb.max_p)
    sn = views.SpaceNormalization(aabb.corners)
    assert np.array_equal(sn.A, pins["aabb/A2"])
    box = sn.normalize_aabb(aabb)
    assert np.isclose(box.longest_extent, 2, rtol=1e-6) and np.allclose(box.center, 0, atol=1e-6)
    v = pins["aabb/points"]
    assert np.allclose(sn.denormalize_mesh(sn.normalize_mesh(v)), v, atol=1e-5)
    vt = sn.normalize_mesh(torch.from_numpy(v))
    assert isinstance(vt, torch.Tensor) and np.allclose(vt.numpy(), sn.normalize_mesh(v), atol=1e-6)


def _project64(K, R, t, x):
    p = x @ R.T + t
    q = p @ K.T
    return q[:, :2] / q[:, 2:], p[:, 2]


def test_normalized_cameras_see_the_moved_space_as_before(pins):
    from garmentdreamer_amd import views
    records = _records(pins)
    sn = views.SpaceNormalization(views.AABB(pins["aabb/points"]).corners)
    A = sn.A.astype(np.float64)
    s = A[0, 0]
    x = np.random.default_rng(11).normal(size=(40, 3))
    for record in records:
        K, R, t = views.camera_from_record(record)
        K = K * 1.7                                                     # K[2,2] != 1: the closed form divides by it
        K2, R2, t2 = views.normalize_camera(K, R, t, sn.A)
        assert K2.dtype == np.float64 and K2[2, 2] == 1 and np.array_equal(R2, R)
        pix, depth = _project64(K, R, t, x)
        pix2, depth2 = _project64(K2, R2, t2, x @ A[:3, :3].T + A[:3, 3])
        assert np.allclose(pix2, pix, rtol=1e-9, atol=0) and np.allclose(depth2, s * depth, rtol=1e-9, atol=0)
    bad = sn.A.copy()
    bad[1, 1] *= 1.5
    with pytest.raises(ValueError, match="A must be a uniform scale"):
        views.normalize_camera(K, R, t, bad)
    sheared = sn.A.copy()
    sheared[0, 1] = 0.01
    with pytest.raises(ValueError, match="A must be a uniform scale"):
        views.normalize_camera(K, R, t, sheared)
    # on views: the float32 camera is the cast of the float64 one
    view = views.View(K, R, t, (16, 16))
    views.SpaceNormalization(views.AABB(pins["aabb/points"]).corners).normalize_views([view])
    assert np.array_equal(view.camera64[2], t2) and np.array_equal(view.t.numpy(), t2.astype(np.float32))
    assert np.allclose(view.center.numpy(), s * (-R.T @ t) + A[:3, 3], atol=1e-5)


# ---- 4. near / far, the sampler, the template ----------------------------------------------------------------------------

def test_near_far_and_mvps(pins):
    from garmentdreamer_amd import views
    from garmentdreamer_amd.mesh_deform import GBufferRenderer
    cams = [views.View(*views.camera_from_record(r), (r["height"], r["width"])) for r in _records(pins)]
    corners = pins["aabb/corners"]
    d = np.stack([np.linalg.norm(corners.astype(np.float64) - v.center.numpy().astype(np.float64), axis=1) for v in cams])
    near, far = views.near_far(cams, corners, epsilon=0.5)
    assert np.isclose(near, 0.5 * d.min(), rtol=1e-5) and np.isclose(far, 1.5 * d.max(), rtol=1e-5)
    assert views.near_far(cams, torch.from_numpy(corners)) == (near, far)
    with pytest.raises(ValueError):
        views.near_far([], corners)
    mvps = views.view_mvps(cams, near, far)
    for v, m in zip(cams, mvps):
        assert torch.equal(m, GBufferRenderer.to_gl_camera(v.K, v.R, v.t, (16, 16), n=near, f=far))
    # project: the pixel of the point the camera looks at from one unit away is the principal point
    v = cams[1]
    ahead = v.center + v.R[2]
    assert torch.allclose(v.project(ahead[None]), torch.tensor([[8.0, 8.0, 1.0]]), atol=1e-4)
    assert torch.allclose(v.project(ahead[None], depth_as_distance=True)[0, 2], torch.tensor(1.0), atol=1e-5)


def test_view_sampler_draws_the_references_positions(pins):
    from garmentdreamer_amd import views
    from tests.golden import make_golden_views as g
    items = [object() for _ in range(g.SAMPLER_VIEWS)]
    for per_iter in (1, 2):
        np.random.seed(g.SAMPLER_SEED)
        s = views.ViewSampler(items, "several", per_iter, g.SAMPLER_PICKED)
        assert s.positions == g.SAMPLER_PICKED and s.views == [items[i] for i in g.SAMPLER_PICKED]
        assert [s() for _ in range(g.SAMPLER_DRAWS)] == pins[f"sampler/several{per_iter}"].tolist()
    np.random.seed(g.SAMPLER_SEED)
    s = views.ViewSampler(items, "all", 1)
    assert [s() for _ in range(g.SAMPLER_DRAWS)] == pins["sampler/all1"].tolist()
    with pytest.raises(ValueError, match="Empty picked_views"):
        views.ViewSampler(items, "several", 1, [])
    with pytest.raises(ValueError, match="Unknown mode"):
        views.ViewSampler(items, "some")


def test_adjust_template():
    from garmentdreamer_amd import views
    v = np.array([[1.0, 2.0, 3.0], [-4.0, 5.0, 0.5]])
    assert np.array_equal(views.adjust_template(v, 0.5), np.array([[1.5, 0.5, 1.0], [0.25, -2.0, 2.5]]))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------

def _capture(tmp_path, n=2, H=6, W=5):
    """a directory of n views in the layout of export.dump_test_view"""
    from garmentdreamer_amd import export
    records = [export.camera_info_entry(vref.rigid_c2w(i + 1), i, W, H, 0.6) for i in range(n)]
    export.save_cameras_json(str(tmp_path / "cameras.json"), records)
    for sub in ("estimated_normals", "gs_rendered_rgba"):
        os.makedirs(tmp_path / sub)
        for i in range(n):
            vref.write_png(tmp_path / sub / f"{i}.png", vref.random_pixels(H, W, 4, i), vref.kinds_for(H, "mixed", i))
    return records


def test_refusals_name_the_file_or_the_argument(tmp_path):
    from garmentdreamer_amd import export, views
    pixels = vref.random_pixels(4, 3, 4, 0)
    # a CPU tensor
    for call, name in ((lambda t: views.png_unfilter(t, 1, 4, 3, 4), "filtered"), (lambda t: views.unpack_rgba(t), "rgba"),
                       (lambda t: views.unpack_view(t, t), "normal_rgba")):
        with pytest.raises(ValueError, match=f"{name} must be a uint8 tensor on the GPU"):
            call(torch.zeros(4 * 13, dtype=torch.uint8))
    # a 16-bit PNG, a row of type 5, a CRC error: before anything is uploaded
    deep = vref.write_png(tmp_path / "deep.png", pixels, [0] * 4, depth=16)
    rows = vref.filter_rows(pixels, [0, 1, 2, 3])
    rows[2, 0] = 5
    five = vref.write_png(tmp_path / "five.png", pixels, None, rows=rows)
    data = bytearray(vref.encode_png(pixels, [4] * 4))
    data[-20] ^= 1                                                      # inside the IDAT chunk's data
    broken = str(tmp_path / "broken.png")
    open(broken, "wb").write(bytes(data))
    for path, what in ((deep, "bit depth 16 is not supported"), (five, "row filter type 5 is not defined"),
                       (broken, "CRC mismatch in the b'IDAT' chunk")):
        with pytest.raises(ValueError) as mine:
            views.decode_png_batch([path])
        assert path in str(mine.value) and what in str(mine.value)
        with pytest.raises(ValueError) as theirs:                       # the same message as the reader they share a parser with
            export.load_image_rgb(path)
        assert str(theirs.value) == str(mine.value)
    # a directory of views
    cap = tmp_path / "capture"
    os.makedirs(cap)
    records = _capture(cap)
    os.rename(cap / "cameras.json", cap / "cameras.txt")
    with pytest.raises(ValueError, match="cameras.json"):
        views.read_views(str(cap))
    with pytest.raises(ValueError, match="cameras.json"):
        views.read_fit_views(str(cap))
    records[1]["img_name"] = "7"
    export.save_cameras_json(str(cap / "cameras.json"), records)
    with pytest.raises(ValueError, match=r"estimated_normals.1\.png.*named '7', not '1'"):
        views.read_views(str(cap))
    with pytest.raises(ValueError, match=r"gs_rendered_rgba.1\.png"):
        views.read_fit_views(str(cap))
    with pytest.raises(ValueError, match="view 5 is not one of the 2 views"):
        views.read_views(str(cap), indices=[5])


def test_mismatched_sizes_are_refused(tmp_path):
    """the sizes are known once the files are inflated, and nothing is uploaded before they agree"""
    from garmentdreamer_amd import views
    _capture(tmp_path)
    vref.write_png(tmp_path / "gs_rendered_rgba" / "1.png", vref.random_pixels(6, 4, 4, 0), [0] * 6)
    with pytest.raises(ValueError, match=r"estimated_normals.1\.png: 5 x 6, but .*gs_rendered_rgba.1\.png is 4 x 6"):
        views.read_views(str(tmp_path))


# ---- 6. the C-ABI ----------------------------------------------------------------------------------------------------

def test_the_bindings_cover_the_header():
    from garmentdreamer_amd import _build, _native
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "gd_views.h")).read()
    declared = set(re.findall(r"^int (gd_views_\w+)\(", header, flags=re.M))
    assert declared == set(_native.VIEWS_SIGNATURES) and len(declared) == 3
    L = _native.lib()
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_views.h but not exported"
        assert getattr(L, name).argtypes == _native.VIEWS_SIGNATURES[name][1]
        assert _native.error_channel(name) == "gd_mesh_last_error"
        count = len(re.search(name + r"\((.*?)\);", header, flags=re.S).group(1).split(","))
        assert count == len(_native.VIEWS_SIGNATURES[name][1]), name
    others = [getattr(_native, n) for n in dir(_native) if n.endswith("SIGNATURES") and n != "VIEWS_SIGNATURES"]
    assert not any(declared & set(t) for t in others)
    assert int(re.search(r"#define GD_VIEWS_MAX_SIDE (\d+)", header).group(1)) == _native.VIEWS_MAX_SIDE
    assert ("raster_views.hip", ["-ffp-contract=off"]) in _build.RASTER_SOURCES


def test_entries_validate_before_any_device_work():
    from garmentdreamer_amd import _native
    L = _native.lib()
    buf = (C.c_uint8 * 64)()
    base = C.addressof(buf)
    p = base + (-base) % 16                                             # 16-byte aligned and never followed
    err = L.gd_mesh_last_error

    def refused(ret, piece):
        assert ret == -1 and piece in err(), err()

    unf, unp, rgba = L.gd_views_png_unfilter, L.gd_views_unpack, L.gd_views_unpack_rgba
    refused(unf(None, None, p, 1, 2, 2, 4), b"png_unfilter: null")
    refused(unf(None, p, None, 1, 2, 2, 4), b"png_unfilter: null")
    for B, H, W in ((0, 2, 2), (1, 0, 2), (1, 2, 0), (1, 8193, 2), (1, 2, 8193), (8193, 2, 2)):
        refused(unf(None, p, p, B, H, W, 4), b"png_unfilter: B, H and W")
    for bpp in (2, 0, 5, 1):
        refused(unf(None, p, p, 1, 2, 2, bpp), b"png_unfilter: bpp")
    refused(unf(None, p, p + 2, 1, 2, 2, 4), b"png_unfilter: filtered and out must be 4-byte aligned")
    refused(unf(None, p + 1, p, 1, 2, 2, 4), b"aligned")
    for k in range(5):
        args = [p, p, 4, p, p, p, 2, 2]
        args[k if k < 2 else k + 1] = None
        refused(unp(None, *args), b"views unpack: null")
    refused(unp(None, p, p, 4, p, p, p, 0, 2), b"views unpack: H and W")
    refused(unp(None, p, p, 4, p, p, p, 2, 8193), b"views unpack: H and W")
    refused(unp(None, p, p, 2, p, p, p, 2, 2), b"3 or 4 channels")
    refused(unp(None, p, p, 4, p, p + 4, p, 2, 2), b"16-byte aligned")
    for k in range(3):
        args = [p, p, p, 2, 2]
        args[k] = None
        refused(rgba(None, *args), b"views unpack_rgba: null")
    refused(rgba(None, p, p, p, 2, 0), b"views unpack_rgba: H and W")
    refused(rgba(None, p + 8, p, p, 2, 2), b"16-byte aligned")
    with pytest.raises(RuntimeError, match=r"gd_views_unpack_rgba failed \(-1\): views unpack_rgba: null pointer"):
        _native.checked("gd_views_unpack_rgba", rgba(None, None, p, p, 2, 2))
