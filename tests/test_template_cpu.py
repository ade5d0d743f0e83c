"""Host side of the template initialisation (garmentdreamer_amd/template.py): the OBJ reader, the seeded area-uniform
surface sampler, and the grid plan of the radius search (gd_scene_shell_grid: host arithmetic, no GPU)."""
import ctypes as C
import math

import numpy as np
import pytest

OBJ = """# a strip of polygons, every corner form
v 0 0 0
v 1 0 0   # trailing comment
v 1 1 0
v 0 1 0
vt 0.5 0.5
vn 0 0 1

v 2 0 0
v 2 1 0
v 3 0.5 0
v 2.5 2 0.25
f 1 2 3
f 1/1 3/1 4/1
f 2//1 5//1 6//1 3//1
f 5/1/1 7/1/1 8/1/1 6/1/1 3/1/1
f -1 -2 -3
"""


def test_load_obj_forms_polygons_and_relative_indices(tmp_path):
    from garmentdreamer_amd.template import load_obj
    p = tmp_path / "strip.obj"
    p.write_text(OBJ)
    v, f = load_obj(str(p))
    assert v.dtype == np.float64 and f.dtype == np.int64
    assert np.array_equal(v, np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0], [2, 1, 0], [3, 0.5, 0],
                                       [2.5, 2, 0.25]], dtype=np.float64))
    assert f.tolist() == [[0, 1, 2], [0, 2, 3],
                          [1, 4, 5], [1, 5, 2],                 # the quad, fan from its first corner
                          [4, 6, 7], [4, 7, 5], [4, 5, 2],      # the pentagon
                          [7, 6, 5]]                            # -1 -2 -3 with 8 vertices read


def test_load_obj_rejects_bad_indices_and_faceless_files(tmp_path):
    from garmentdreamer_amd.template import load_obj
    for name, text in (("high", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n"), ("low", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -4\n"),
                       ("zero", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n")):
        p = tmp_path / (name + ".obj")
        p.write_text(text)
        with pytest.raises(ValueError, match="out of range|index 0"):
            load_obj(str(p))
    p = tmp_path / "points.obj"
    p.write_text("# only vertices\nv 0 0 0\nv 1 0 0\nv 0 1 0\n")
    with pytest.raises(ValueError, match="no faces"):
        load_obj(str(p))


def _barycentric(p, a, b, c):
    """(w [n,3], off-plane distance [n]) of points p against triangles (a, b, c), float64."""
    e0, e1 = b - a, c - a
    nrm = np.cross(e0, e1)
    nrm = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
    d = p - a
    off = np.abs((d * nrm).sum(-1))
    d00, d01, d11 = (e0 * e0).sum(-1), (e0 * e1).sum(-1), (e1 * e1).sum(-1)
    d20, d21 = (d * e0).sum(-1), (d * e1).sum(-1)
    den = d00 * d11 - d01 * d01
    w1 = (d11 * d20 - d01 * d21) / den
    w2 = (d00 * d21 - d01 * d20) / den
    return np.stack((1.0 - w1 - w2, w1, w2), axis=-1), off


def test_sample_surface_lies_on_triangles_in_proportion_to_area():
    from garmentdreamer_amd.template import sample_surface
    # areas 1 : 3 in two different planes, and a zero-area triangle between them in the face list
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0],
                  [5, 0, 1], [5, 3, 1], [5, 0, 3],
                  [1, 1, 5], [2, 2, 6], [3, 3, 7]], dtype=np.float64)
    f = np.array([[0, 1, 2], [6, 7, 8], [3, 4, 5]], dtype=np.int64)
    n = 40000
    p = sample_surface(v, f, n, seed=3)
    assert p.shape == (n, 3) and p.dtype == np.float64
    inside = []
    for t in (0, 2):
        w, off = _barycentric(p, *(v[f[t, k]] for k in range(3)))
        inside.append((w.min(axis=1) >= -1e-12) & (w.max(axis=1) <= 1 + 1e-12) & (off <= 1e-12))
    assert np.all(inside[0] ^ inside[1])           # every sample on exactly one of the two real triangles
    on_line = np.linalg.norm(np.cross(p - v[6], v[7] - v[6]), axis=1) <= 1e-12
    assert not on_line.any()                       # none on the degenerate one
    sigma = math.sqrt(n * 0.25 * 0.75)             # binomial, p = 1/4
    assert abs(int(inside[0].sum()) - n // 4) <= 4 * sigma, int(inside[0].sum())


def test_sample_surface_is_seeded_and_leaves_the_global_generator_alone():
    from garmentdreamer_amd.template import sample_surface
    rng = np.random.RandomState(5)
    v = rng.normal(size=(30, 3))
    f = np.stack([rng.permutation(30)[:3] for _ in range(50)])
    np.random.seed(1234)
    before = np.random.get_state()
    a = sample_surface(v, f, 1000, seed=7)
    b = sample_surface(v, f, 1000, seed=7)
    c = sample_surface(v, f, 1000, seed=8)
    after = np.random.get_state()
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    # every sample inside some triangle of the mesh
    ok = np.zeros(1000, dtype=bool)
    for t in range(f.shape[0]):
        w, off = _barycentric(a, *(v[f[t, k]] for k in range(3)))
        ok |= (w.min(axis=1) >= -1e-12) & (off <= 1e-12)
    assert ok.all()


def _plan(lo, hi, radius):
    from garmentdreamer_amd import _native
    L = _native.lib()
    edge, dims = C.c_float(-1.0), (C.c_int * 3)(-1, -1, -1)
    ret = L.gd_scene_shell_grid((C.c_float * 3)(*lo), (C.c_float * 3)(*hi), radius, C.byref(edge), dims)
    return ret, edge.value, tuple(dims), L.gd_scene_last_error()


CAP = 1 << 24


def test_shell_grid_plan():
    box = ((-1.0, 0.0, 0.25), (1.0, 1.0, 0.75))                 # 2 x 1 x 0.5
    ret, edge, dims, _ = _plan(*box, 3.0)                        # radius beyond the extent: one cell
    assert ret == 0 and dims == (1, 1, 1) and edge == 3.0
    ret, edge, dims, _ = _plan(*box, 0.01)
    assert ret == 0 and edge == np.float32(0.01)
    assert all(abs(d - e) <= 1 for d, e in zip(dims, (200, 100, 50))), dims
    ret, edge, dims, _ = _plan(*box, 1e-5)                       # the cap: the edge grows past the radius
    assert ret == 0 and edge > 1e-5 and min(dims) >= 1 and dims[0] * dims[1] * dims[2] <= CAP
    assert dims[0] >= 255                                        # ... and no further than the cap asks
    ret, edge, dims, _ = _plan((0.0, 0.0, 2.0), (1.0, 1.0, 2.0), 0.1)     # flat box
    assert ret == 0 and dims[2] == 1 and dims[0] in (10, 11) and dims[1] in (10, 11)
    ret, edge, dims, _ = _plan((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 0.5)     # a single point
    assert ret == 0 and dims == (1, 1, 1) and edge == 0.5


def test_shell_arguments_are_validated_before_any_device_work():
    from garmentdreamer_amd import _native
    L = _native.lib()
    box = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    for radius in (-0.1, 0.0, float("nan"), float("inf")):
        ret, _, _, msg = _plan(*box, radius)
        assert ret == -1 and b"radius" in msg, (radius, msg)
    ret, _, _, msg = _plan((0.0, 0.0, 0.0), (1.0, -1.0, 1.0), 0.1)
    assert ret == -1 and b"bounding box" in msg
    lo, hi = (C.c_float * 3)(*box[0]), (C.c_float * 3)(*box[1])
    assert L.gd_scene_shell_search(None, -1, None, 4, None, lo, hi, 0.1, None, None, None) == -1
    assert b"S must be" in L.gd_scene_last_error()
    assert L.gd_scene_shell_search(None, 4, None, -1, None, lo, hi, 0.1, None, None, None) == -1
    assert b"Q must be" in L.gd_scene_last_error()
    assert L.gd_scene_shell_search(None, 4, None, 4, None, lo, hi, float("nan"), None, None, None) == -1
    assert b"radius" in L.gd_scene_last_error()
    assert L.gd_scene_shell_search(None, 4, None, 4, None, lo, hi, 0.1, None, None, None) == -1      # null pointers
    assert L.gd_scene_shell_search(None, 4, None, 0, None, lo, hi, 0.1, None, None, None) == 0       # nothing to do
    with pytest.raises(RuntimeError, match="gd_scene_shell_grid failed.*radius"):
        _native.check_scene(L.gd_scene_shell_grid(lo, hi, -1.0, None, None), "gd_scene_shell_grid")
    assert L.gd_scene_shell_scratch_bytes(50000, 200 * 100 * 50) >= 4 * 200 * 100 * 50 + 16 * 50000


def test_shell_search_rejects_cpu_tensors():
    import torch
    from garmentdreamer_amd.template import shell_search
    with pytest.raises(RuntimeError, match="no CPU path"):
        shell_search(torch.zeros(4, 3), torch.zeros(5, 3), 0.1)
