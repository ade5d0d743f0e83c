"""GPU parity of the template initialisation: the fixed-radius nearest-sample search (csrc/raster_template.hip,
gd_scene_shell_search) bit for bit against an fp32 numpy brute force with the same operation order and tie rule, its
accept / reject decision against the reference's float64 rule, ``template_point_cloud`` against a numpy restatement of
its seven steps, and ``GaussianModel.create_from_template`` through one loop step.

The mesh is generated: an open tube of 24 x 12 quads, radius 0.3, height 1."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RADIUS = 0.02


def _tube(nu=24, nv=12, r=0.3, h=1.0):
    """(vertices [V,3], quads [nu * nv, 4]) of an open tube around the z axis."""
    ang = 2.0 * np.pi * np.arange(nu) / nu
    v = np.array([[r * np.cos(a), r * np.sin(a), h * j / nv] for j in range(nv + 1) for a in ang], dtype=np.float64)
    quads = np.array([[j * nu + i, j * nu + (i + 1) % nu, (j + 1) * nu + (i + 1) % nu, (j + 1) * nu + i]
                      for j in range(nv) for i in range(nu)], dtype=np.int64)
    return v, quads


def _tube_triangles():
    v, q = _tube()
    return v, np.concatenate((q[:, [0, 1, 2]], q[:, [0, 2, 3]]))


def _write_tube_obj(path):
    v, q = _tube()
    with open(path, "w") as f:
        f.write("# generated tube\n")
        for p in v:
            f.write("v %r %r %r\n" % tuple(float(x) for x in p))
        for c in q:
            f.write("f %d %d %d %d\n" % tuple(int(i) + 1 for i in c))


def _samples(S, seed=1):
    from garmentdreamer_amd.template import sample_surface
    return sample_surface(*_tube_triangles(), S, seed).astype(np.float32)


def _box_queries(Q, seed, lo=None, hi=None):
    """Uniform in the bounding box of the tube MESH (for a handful of samples that is wider than the samples' own box,
    so some queries lie outside the grid)."""
    v, _ = _tube()
    lo = v.min(axis=0) if lo is None else lo
    hi = v.max(axis=0) if hi is None else hi
    return np.random.RandomState(seed).uniform(lo, hi, size=(Q, 3)).astype(np.float32)


def brute_fp32(s, q, radius):
    """(nearest, dist2) by the kernel's rules in numpy fp32: d2 = (dx dx + dy dy) + dz dz, one rounding per operation,
    argmin takes the first (= lowest) index among equal d2, accepted if d2 < fl(radius radius)."""
    assert s.dtype == np.float32 and q.dtype == np.float32
    r = np.float32(radius)
    r2 = r * r
    idx = np.empty(q.shape[0], dtype=np.int64)
    best = np.empty(q.shape[0], dtype=np.float32)
    step = max(1, (8 << 20) // max(1, s.shape[0]))            # 8 M pairs = 32 MB per fp32 temporary
    for a in range(0, q.shape[0], step):
        qq = q[a:a + step]
        dx = qq[:, None, 0] - s[None, :, 0]
        dy = qq[:, None, 1] - s[None, :, 1]
        dz = qq[:, None, 2] - s[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        i = d2.argmin(axis=1)
        idx[a:a + step] = i
        best[a:a + step] = d2[np.arange(d2.shape[0]), i]
    return np.where(best < r2, idx, -1).astype(np.int32), best


def nearest_fp64(s, q):
    """(index, distance) of the nearest sample in float64 on the same float32 values."""
    s64, q64 = s.astype(np.float64), q.astype(np.float64)
    idx = np.empty(q.shape[0], dtype=np.int64)
    dist = np.empty(q.shape[0], dtype=np.float64)
    step = max(1, (4 << 20) // max(1, s.shape[0]))
    for a in range(0, q.shape[0], step):
        qq = q64[a:a + step]
        d2 = (qq[:, None, 0] - s64[None, :, 0]) ** 2
        d2 += (qq[:, None, 1] - s64[None, :, 1]) ** 2
        d2 += (qq[:, None, 2] - s64[None, :, 2]) ** 2
        i = d2.argmin(axis=1)
        idx[a:a + step] = i
        dist[a:a + step] = np.sqrt(d2[np.arange(d2.shape[0]), i])
    return idx, dist


def gpu_search(s, q, radius):
    from garmentdreamer_amd.template import shell_search
    n, d = shell_search(torch.from_numpy(s).to(DEV), torch.from_numpy(q).to(DEV), radius)
    assert n.dtype == torch.int32 and d.dtype == torch.float32 and n.shape == d.shape == (q.shape[0],)
    return n.cpu().numpy(), d.cpu().numpy()


def assert_matches_brute(s, q, radius):
    ref_n, ref_d = brute_fp32(s, q, radius)
    out_n, out_d = gpu_search(s, q, radius)
    assert np.array_equal(out_n, ref_n), int((out_n != ref_n).sum())
    acc = ref_n >= 0
    assert np.array_equal(out_d[acc].view(np.uint32), ref_d[acc].view(np.uint32))
    # a rejected query reports the minimum over the cells it visited: never below the true minimum
    assert np.all(out_d[~acc] >= ref_d[~acc])
    return out_n, out_d, ref_d


@functools.lru_cache(maxsize=None)
def _case(S, Q):
    """One (samples, queries, brute force) set per shape, shared by the tests that need it; treated as read-only."""
    s, q = _samples(S), _box_queries(Q, seed=100 + S)
    return s, q, brute_fp32(s, q, RADIUS)


@pytest.mark.parametrize("S,Q", [(1, 1), (7, 255), (300, 257), (2000, 20000)])
def test_shell_search_bit_exact_vs_fp32_brute_force(S, Q):
    s, q, (ref_n, ref_d) = _case(S, Q)
    out_n, out_d = gpu_search(s, q, RADIUS)
    assert np.array_equal(out_n, ref_n), int((out_n != ref_n).sum())
    acc = ref_n >= 0
    assert np.array_equal(out_d[acc].view(np.uint32), ref_d[acc].view(np.uint32))
    assert np.all(out_d[~acc] >= ref_d[~acc])
    if S >= 2000:
        assert 0 < acc.sum() < Q                  # both outcomes occur
    again_n, again_d = gpu_search(s, q, RADIUS)   # reruns are bit-identical, rejected queries included
    assert np.array_equal(again_n, out_n) and np.array_equal(again_d.view(np.uint32), out_d.view(np.uint32))


def test_duplicated_samples_resolve_to_the_lower_index():
    s = _samples(800).copy()
    n = s.shape[0] // 8
    s[n:2 * n] = s[:n]                                          # every one of the first n samples exists twice
    rng = np.random.RandomState(7)
    q = np.concatenate((_box_queries(3000, seed=8), s[rng.randint(0, 2 * n, size=1000)] +
                        rng.normal(scale=0.004, size=(1000, 3)).astype(np.float32)))
    out_n, _, _ = assert_matches_brute(s, q, RADIUS)
    assert (out_n >= 0).sum() > 500 and ((out_n >= 0) & (out_n < n)).sum() > 100
    assert not ((out_n >= n) & (out_n < 2 * n)).any()           # the copy never wins a tie


def test_queries_equal_to_samples_are_accepted_at_distance_zero():
    s = _samples(1500)
    out_n, out_d, _ = assert_matches_brute(s, s.copy(), RADIUS)
    assert np.array_equal(out_d, np.zeros_like(out_d))
    assert np.array_equal(out_n, np.arange(s.shape[0], dtype=np.int32))      # distinct samples: each finds itself


def test_queries_on_the_upper_faces_and_outside_the_box():
    s = _samples(1000)
    lo, hi = s.min(axis=0), s.max(axis=0)
    rng = np.random.RandomState(9)
    face = rng.uniform(lo, hi, size=(1500, 3)).astype(np.float32)
    for k in range(3):
        face[k::3, k] = hi[k]                                    # on the upper face of axis k
        face[k:300:3, (k + 1) % 3] = hi[(k + 1) % 3]             # some on an edge of the box
    face[:8] = hi                                                # and the upper corner itself
    wide = rng.uniform(lo - 3 * RADIUS, hi + 3 * RADIUS, size=(6000, 3)).astype(np.float32)
    outside = wide[np.any((wide < lo) | (wide > hi), axis=1)]
    # samples on the boundary of the box, pushed outwards by less than the radius: accepted from outside
    edge_s = s[np.argsort(-s[:, 2])[:200]]
    near_out = edge_s + np.array([0, 0, 0.5 * RADIUS], dtype=np.float32)
    q = np.concatenate((face, outside, near_out))
    assert outside.shape[0] > 500
    out_n, _, _ = assert_matches_brute(s, q, RADIUS)
    assert (out_n[:1500] >= 0).any() and (out_n[-200:] >= 0).all()


def test_radius_beyond_the_extent_is_a_single_cell():
    s, q = _samples(300), _box_queries(257, seed=10)
    out_n, _, _ = assert_matches_brute(s, q, 5.0)
    assert (out_n >= 0).all()


def test_radius_too_small_to_accept_anything():
    s, q = _samples(300), _box_queries(2000, seed=11)
    out_n, _, _ = assert_matches_brute(s, q, 1e-7)
    assert (out_n == -1).all()


def test_radius_that_hits_the_cell_cap():
    import ctypes as C
    from garmentdreamer_amd import _native
    s = _samples(2000)
    radius = 0.002                                               # extent 1 / 255 cells = 0.0039 > radius
    rng = np.random.RandomState(12)
    q = np.concatenate((s[rng.randint(0, s.shape[0], size=4000)] + rng.normal(scale=0.0012, size=(4000, 3)).astype(np.float32),
                        _box_queries(4000, seed=13)))
    edge, dims = C.c_float(0), (C.c_int * 3)()
    lo, hi = (C.c_float * 3)(*s.min(axis=0).tolist()), (C.c_float * 3)(*s.max(axis=0).tolist())
    assert _native.lib().gd_scene_shell_grid(lo, hi, radius, C.byref(edge), dims) == 0
    assert edge.value > radius and max(dims) >= 255 and dims[0] * dims[1] * dims[2] <= 1 << 24
    out_n, _, _ = assert_matches_brute(s, q, radius)
    assert 500 < (out_n[:4000] >= 0).sum() < 3500


def test_decision_agrees_with_the_float64_rule_outside_a_derived_band():
    """The reference accepts when ||p - nearest||_2 < deviation in float64.  The fp32 kernel forms three differences,
    three squares, two sums and radius^2, each within 2^-24 relative: d2 within about 5 * 2^-24, d within about 1.5e-7
    relative.  A band of 1e-6 * deviation around the threshold leaves a factor of six; outside it the two decisions
    must be the same.  That few queries fall inside the band is a condition on the input (float64 oracle alone)."""
    s, q, _ = _case(2000, 20000)
    out_n, _ = gpu_search(s, q, RADIUS)
    _, d64 = nearest_fp64(s, q)
    band = np.abs(d64 - RADIUS) <= 1e-6 * RADIUS
    assert band.mean() <= 1e-3, band.mean()
    assert np.array_equal((out_n >= 0)[~band], (d64 < RADIUS)[~band])


def _numpy_template(path, num_pts, num_pts_space, deviation, radius=4.0, scale=0.4, seed=0):
    """The seven steps of template_point_cloud in numpy, nearest search in float64.  Returns what the comparison needs."""
    from garmentdreamer_amd.scene import SH_C0
    from garmentdreamer_amd.template import load_obj, sample_surface
    v, f = load_obj(path)
    smp = sample_surface(v, f, num_pts, seed)
    coords = np.stack((smp[:, 2], smp[:, 0], smp[:, 1]), axis=1)                        # 1. (z, x, y)
    rgb = np.random.RandomState(seed + 1).random((num_pts, 3)) / 255.0 * SH_C0 + 0.5    # 2.
    stream = np.random.RandomState(0)
    cand = stream.uniform(low=coords.min(axis=0), high=coords.max(axis=0), size=(num_pts_space, 3))   # 3.
    s32, c32 = coords.astype(np.float32), cand.astype(np.float32)
    near, d64 = nearest_fp64(s32, c32)                                                  # 4.
    return dict(s32=s32, c32=c32, rgb=rgb, near=near, d64=d64, stream=stream, bound=radius * scale)


def test_template_point_cloud_end_to_end(tmp_path):
    from garmentdreamer_amd.template import template_point_cloud
    path = str(tmp_path / "tube.obj")
    _write_tube_obj(path)
    num_pts, num_space, dev_ = 2000, 20000, 0.02
    pts, cols, bound = template_point_cloud(path, num_pts=num_pts, num_pts_space=num_space, deviation=dev_, device=DEV)
    assert bound == 1.6 and pts.dtype == cols.dtype == torch.float32 and pts.is_cuda and cols.is_cuda
    assert pts.shape == cols.shape and pts.shape[1] == 3
    ref = _numpy_template(path, num_pts, num_space, dev_)
    b32 = np.float32(ref["bound"])
    P = pts.shape[0]
    n_acc = P - num_pts
    pts_h, cols_h = pts.cpu().numpy(), cols.cpu().numpy()
    # the trailing rows: the permuted samples and their colours
    assert np.array_equal(pts_h[n_acc:], ref["s32"] * b32)
    assert np.allclose(cols_h[n_acc:], ref["rgb"], rtol=0, atol=1e-6)
    # 5. the accepted candidates, in candidate order; only inside the band may the set differ from the float64 rule
    band = np.abs(ref["d64"] - dev_) <= 1e-6 * dev_
    assert band.mean() <= 1e-3
    cand_b = np.ascontiguousarray(ref["c32"] * b32)
    row = lambda a: np.ascontiguousarray(a).view([("", np.float32)] * 3).ravel()         # noqa: E731
    assert np.unique(row(cand_b)).shape[0] == num_space
    mask = np.isin(row(cand_b), row(pts_h[:n_acc]))
    assert mask.sum() == n_acc and np.array_equal(cand_b[mask], pts_h[:n_acc])
    assert np.array_equal(mask[~band], (ref["d64"] < dev_)[~band])
    assert 0 < n_acc < num_space
    # 6. colours: the nearest sample's + 0.2 * the continuing stream
    jitter = 0.2 * ref["stream"].random((n_acc, 3))
    want = ref["rgb"][ref["near"][mask]] + jitter
    bad = np.flatnonzero(np.abs(cols_h[:n_acc] - want).max(axis=1) > 1e-6)
    # where two samples are equally near within the band the index may differ: such a row must carry the colour of
    # SOME sample that is as near as the nearest, within the band
    s64 = ref["s32"].astype(np.float64)
    for i in bad:
        c = ref["c32"][mask][i].astype(np.float64)
        d = np.sqrt(((s64 - c) ** 2).sum(axis=1))
        tied = np.flatnonzero(d <= d.min() * (1 + 1e-6))
        assert any(np.abs(cols_h[i] - (ref["rgb"][j] + jitter[i])).max() <= 1e-6 for j in tied), (i, tied)
    assert bad.shape[0] <= 1e-3 * n_acc
    # a second call returns the same bits
    pts2, cols2, _ = template_point_cloud(path, num_pts=num_pts, num_pts_space=num_space, deviation=dev_, device=DEV)
    assert torch.equal(pts, pts2) and torch.equal(cols, cols2)


def test_template_point_cloud_default_bound(tmp_path):
    from garmentdreamer_amd.template import template_point_cloud
    path = str(tmp_path / "tube.obj")
    _write_tube_obj(path)
    pts, cols, bound = template_point_cloud(path, num_pts=500, num_pts_space=2000, device=DEV)    # default deviation 0.01
    assert bound == 1.6 and pts.shape[0] >= 500 and pts.shape == cols.shape


def test_create_from_template_and_one_loop_step(tmp_path):
    from garmentdreamer_amd import cameras as gcam, gaussian_model as gm
    from garmentdreamer_amd.sds_loop import SDSLoop
    from garmentdreamer_amd.template import template_point_cloud
    path = str(tmp_path / "tube.obj")
    _write_tube_obj(path)
    kw = dict(num_pts=2000, num_pts_space=20000, deviation=0.02)
    pts, _, bound = template_point_cloud(path, device=DEV, **kw)
    m = gm.GaussianModel(sh_degree=0, device=DEV)
    assert m.create_from_template(path, spatial_lr_scale=4.0, **kw) == bound
    assert m._xyz.shape[0] == pts.shape[0] > kw["num_pts"] and m.spatial_lr_scale == 4.0
    assert torch.equal(m._xyz.data, pts)
    sc = m.get_scaling
    assert torch.isfinite(sc).all() and (sc > 0).all()
    ply = str(tmp_path / "template.ply")
    m.save_ply(ply)
    m2 = gm.GaussianModel(sh_degree=0, device=DEV)
    m2.load_ply(ply)
    assert torch.equal(m2._xyz.data, m._xyz.data)
    m.training_setup()

    class ToyGuidance:   # the stand-in of tests/test_scene_gpu.py (local to its test there): pulls the render towards grey
        def __call__(self, rgb, *a, **k):
            return {"loss_sds": ((rgb - 0.5) ** 2).sum() / rgb.shape[0], "grad_norm": torch.zeros((), device=rgb.device)}

        def set_min_max_steps(self, **k):
            pass

    loop = SDSLoop(m, ToyGuidance(), None, torch.ones(3, device=DEV))
    out = loop.step(gcam.orbit_batch(2, elevation_deg=15.0, camera_distance=2.75, fovy_deg=55.0, height=64, width=64))
    assert torch.isfinite(out["loss"]) and torch.isfinite(m.flat_grad).all() and m.flat_grad.abs().sum() > 0
    assert torch.isfinite(m._flat).all()


def test_shell_search_has_no_cpu_path():
    from garmentdreamer_amd.template import shell_search
    with pytest.raises(RuntimeError, match="no CPU path"):
        shell_search(torch.zeros(4, 3), torch.zeros(5, 3), 0.1)
