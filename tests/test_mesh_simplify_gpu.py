"""GPU checks of the final-mesh post-process (garmentdreamer_amd/mesh_simplify.py, the entries of include/gd_mesh_simplify.h
in csrc/raster_simplify.hip) and of ``Deformer.final_mesh`` against the numpy statement of tests/simplify_reference.py.

Decimation is fp64 IEEE adds and multiplies in a fixed order on both sides, built without contraction: quadrics, costs, keys,
the selection of every pass and so the faces, vertices and ``info`` of whole decimations must EQUAL the statement's, bit for
bit.  Taubin smoothing is fp32 and follows the 4x rule of test_mesh_geometry_gpu._check: the GPU's normalised error against
the float64 statement is at most four times the float32 statement's own.

Meshes: those of tests/remesh_reference.py (a triangle, a quad, the 200-face cloth, the 576-face tube: several workgroups per
edge kernel, the closed 128-face sphere, the cloth with an unreferenced vertex), a tetrahedron, an octahedron, the 6 x 6
integer grid and the folded sheet.  The longest runs are some 30 rounds."""
import functools

import numpy as np
import pytest
import torch

from tests import remesh_reference as rr
from tests import simplify_reference as sr
from tests.test_mesh_geometry_gpu import _check, _deformer
from tests.test_mesh_simplify_cpu import TARGETS, decimated, noisy_sphere, target_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gpu_mesh(v, tri):
    return _dev(v.astype(np.float32)), _dev(tri.astype(np.int32))


def _ms():
    from garmentdreamer_amd import mesh_simplify as ms
    return ms


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _assert_same_bits(what, got, want):
    """fp64 arrays, bit for bit; the message carries the largest difference in units of the last place"""
    g, w = _bits(got), _bits(np.asarray(want, dtype=np.float64))
    if not np.array_equal(g, w):
        ulps = np.abs(g.astype(np.float64) - w.astype(np.float64))     # same sign and finite: the bit patterns are ordered
        raise AssertionError(f"{what}: {int((g != w).sum())} of {g.size} values differ, by at most {ulps.max():.0f} ulps "
                             f"(at flat index {int(ulps.argmax())})")


@functools.lru_cache(maxsize=None)
def _first_round(name):
    """the statement's connectivity, quadrics and first round to half the faces; shared and read-only"""
    v, tri = sr.mesh(name)
    c = rr.Connectivity(tri, v.shape[0])
    q = sr.vertex_quadrics(v, c)
    trace, q_after = {}, q.copy()
    t2, n = sr.decimation_round(v.astype(np.float64), tri, q_after, tri.shape[0] // 2, trace=trace)
    return dict(v=v, tri=tri, c=c, q=q, q_after=q_after, tri_after=t2, selected=n, **trace)


def _gpu_first_round(name):
    from garmentdreamer_amd import mesh_remesh as mr
    ms, s = _ms(), _first_round(name)
    gv, gt = _gpu_mesh(s["v"], s["tri"])
    conn = mr.build_connectivity(gt, gv.shape[0])
    assert np.array_equal(conn.ev.cpu().numpy(), s["c"].ev)
    q = ms.vertex_quadrics(gv, conn)
    key, direction, cost = ms.collapse_candidates(gv, conn, q)
    return gv, gt, conn, q, key, direction, cost


# ---- quadrics, costs, keys ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cloth", "tube", "sphere", "integer"])
def test_quadrics_costs_and_keys_equal_the_statement_bit_for_bit(name):
    s = _first_round(name)
    _, _, _, q, key, direction, cost = _gpu_first_round(name)
    assert q.dtype == torch.float64 and cost.dtype == torch.float64 and key.dtype == torch.int64
    _assert_same_bits(f"{name} vertex quadrics", q, s["q"])
    _assert_same_bits(f"{name} first-round costs", cost, s["costs"])
    assert direction.cpu().tolist() == s["direction"] and key.cpu().tolist() == s["keys"]
    assert sum(d != 0 for d in s["direction"]) > 0 and {1, 2} <= set(s["direction"])
    if name == "integer":
        assert np.array_equal(s["q"], np.round(s["q"])) and np.array_equal(s["costs"], np.round(s["costs"]))
        live = [s["keys"][e] >> 32 for e in s["live"]]
        assert len(set(live)) < len(live)                              # equal costs among the live: the edge index decides


@pytest.mark.parametrize("name", sr.MESHES)
def test_one_round_equals_the_statement(name):
    ms, s = _ms(), _first_round(name)
    from garmentdreamer_amd import mesh_remesh as mr
    gv, gt = _gpu_mesh(s["v"], s["tri"])
    conn = mr.build_connectivity(gt, gv.shape[0])
    q = ms.vertex_quadrics(gv, conn)
    out, n = ms.decimation_round(gv, gt, q, s["tri"].shape[0] // 2, 4, conn)
    print(name, "selected", n, "per pass", [len(w) for w in s["winners"]], "faces", s["tri"].shape[0], "->", out.shape[0])
    assert n == s["selected"] and np.array_equal(out.cpu().numpy(), s["tri_after"])
    _assert_same_bits(f"{name} quadrics after the round", q, s["q_after"])
    if name in ("cloth", "tube", "sphere", "folded"):
        assert n > 0 and sum(len(w) > 0 for w in s["winners"]) > 1       # a later pass did select


# ---- whole decimations --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _gpu_decimated(name, kind):
    v, tri = sr.mesh(name)
    return _ms().decimate_quadric(*_gpu_mesh(v, tri), target_of(name, kind))


@pytest.mark.parametrize("kind", TARGETS)
@pytest.mark.parametrize("name", sr.MESHES)
def test_whole_decimation_equals_the_statement(name, kind):
    v2, t2, info = decimated(name, kind)
    gv, gt, ginfo = _gpu_decimated(name, kind)
    print(f"{name} {kind}: {sr.mesh(name)[1].shape[0]} -> {gt.shape[0]} faces, info {ginfo}")
    assert gv.dtype == torch.float32 and gt.dtype == torch.int32 and gv.is_cuda and gt.is_cuda
    assert ginfo == info and type(ginfo["reached"]) is bool and all(type(n) is int for n in ginfo["selected"] + ginfo["faces"])
    assert np.array_equal(gt.cpu().numpy(), t2)
    assert np.array_equal(_bits(gv), _bits(v2))


def test_two_runs_are_bit_identical():
    v, tri = sr.mesh("tube")
    first = _gpu_decimated("tube", "quarter")
    gv, gt, info = _ms().decimate_quadric(*_gpu_mesh(v, tri), target_of("tube", "quarter"))
    assert torch.equal(gv.view(torch.int32), first[0].view(torch.int32)) and torch.equal(gt, first[1]) and info == first[2]


def test_the_unreferenced_vertex_is_dropped_and_a_small_mesh_comes_back_as_copies():
    v, tri = sr.mesh("cloth_extra")
    gv, gt, _ = _gpu_decimated("cloth_extra", "half")
    assert gv.shape[0] == int(torch.unique(gt).numel()) and not (gv == _dev(v[7])).all(dim=1).any()
    iv, it = _gpu_mesh(v, tri)
    ov, ot, info = _ms().decimate_quadric(iv, it, tri.shape[0])
    assert torch.equal(ov, iv) and torch.equal(ot, it) and ov.data_ptr() != iv.data_ptr() and ot.data_ptr() != it.data_ptr()
    assert info == {"reached": True, "selected": [], "faces": []}
    tv, tt = _gpu_mesh(*sr.mesh("tetrahedron"))                        # a run that selects nothing: copies too
    ov, ot, info = _ms().decimate_quadric(tv, tt, 2)
    assert torch.equal(ov, tv) and torch.equal(ot, tt) and ov.data_ptr() != tv.data_ptr() and ot.data_ptr() != tt.data_ptr()
    assert info == {"reached": False, "selected": [0], "faces": [4]}


def test_max_rounds_ends_a_run():
    v, tri = sr.mesh("cloth")
    _, t2, info = sr.decimate(v, tri, 50, max_rounds=3)
    gv, gt, ginfo = _ms().decimate_quadric(*_gpu_mesh(v, tri), 50, max_rounds=3)
    assert ginfo == info and not info["reached"] and len(info["selected"]) == 3 and np.array_equal(gt.cpu().numpy(), t2)


# ---- Taubin smoothing -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["cloth", "tube", "noisy_sphere", "cloth_extra", "quad"])
@pytest.mark.parametrize("steps,mu", [(1, 0.0), (10, -0.53)])
def test_taubin_against_the_float64_statement(name, steps, mu):
    """(1, 0.0) is ONE pass: a pass with weight 0 returns p + 0 (mean - p) = p exactly"""
    v, tri = noisy_sphere() if name == "noisy_sphere" else sr.mesh(name)
    r64 = sr.taubin(v, tri, steps, 0.5, mu, dtype=np.float64)
    r32 = sr.taubin(v, tri, steps, 0.5, mu, dtype=np.float32)
    gv, gt = _gpu_mesh(v, tri)
    before = gv.clone()
    got = _ms().taubin_smooth(gv, gt, steps, 0.5, mu)
    assert got.dtype == torch.float32 and got.shape == gv.shape and torch.equal(gv, before) and got.data_ptr() != gv.data_ptr()
    same = np.array_equal(_bits(got), _bits(r32))
    print(f"{name} taubin steps {steps} mu {mu}: bit-equal to the float32 statement: {same}")
    if np.array_equal(r32.astype(np.float64), r64):
        assert same                                                    # nothing rounds: there is no error to compare
    else:
        _check(f"{name} taubin {steps}", got.cpu().numpy(), r64, r32)
    c = rr.Connectivity(tri, v.shape[0])
    if name == "tube":
        assert torch.equal(got[_dev(c.bnd)][:, 2], gv[_dev(c.bnd)][:, 2])     # the rims stay in their planes
    if name == "cloth_extra":
        assert torch.equal(got[7], gv[7])                              # an isolated vertex stays
    assert torch.equal(_ms().taubin_smooth(gv, gt, steps, 0.5, mu), got)


# ---- the final mesh ---------------------------------------------------------------------------------------------------------

def test_post_process_mesh_on_the_tube():
    ms = _ms()
    v, tri = sr.mesh("tube")
    gv, gt = _gpu_mesh(v, tri)
    rot = ms.rotate_upright(gv)
    assert np.array_equal(_bits(rot), _bits(sr.rotate(v)))
    dv, dt, dinfo = ms.post_process_mesh(gv, gt, 144, smooth=False)
    sv, st, sinfo = sr.post_process(v, tri, 144, smooth=False)
    assert dinfo == sinfo and dinfo["reached"] and 143 <= dt.shape[0] <= 144
    assert np.array_equal(dt.cpu().numpy(), st) and np.array_equal(_bits(dv), _bits(sv))
    assert sr.boundary_of(dv.cpu().numpy(), st) == sr.boundary_of(sr.rotate(v), tri)      # the rotated input rim, exactly
    ov, ot, info = ms.post_process_mesh(gv, gt, 144)
    assert torch.equal(ot, dt) and info == dinfo
    out_v, out_t = ov.cpu().numpy(), ot.cpu().numpy().astype(np.int64)
    assert rr.invariants(out_v, out_t) == rr.invariants(v, tri)
    _check("tube post-process", out_v, sr.taubin(sv, st, dtype=np.float64), sr.taubin(sv, st, dtype=np.float32))
    c = rr.Connectivity(out_t, out_v.shape[0])
    assert set(out_v[c.bnd, 1].tolist()) == {0.0, 1.0}                  # the rims, now in the planes y = 0 and y = 1
    nv, nt, ninfo = ms.post_process_mesh(gv, gt, 144, smooth=False, rotate=False)
    pv, pt, pinfo = sr.post_process(v, tri, 144, smooth=False, do_rotate=False)
    assert ninfo == pinfo and np.array_equal(nt.cpu().numpy(), pt) and np.array_equal(_bits(nv), _bits(pv))


def test_deformer_final_mesh_leaves_the_deformer_unchanged(tmp_path):
    from garmentdreamer_amd import template
    ms = _ms()
    d = _deformer()
    for _ in range(2):
        d.step([0, 1])
    state = (d.initial.clone(), d.offsets.detach().clone(), d.geometry.tri.clone(), d.geometry, d.offsets, d.optimizer, d.lr)
    fv, ft = d.final_mesh(target_faces=200)
    assert torch.equal(d.initial, state[0]) and torch.equal(d.offsets.detach(), state[1])
    assert torch.equal(d.geometry.tri, state[2])
    assert d.geometry is state[3] and d.offsets is state[4] and d.optimizer is state[5] and d.lr == state[6]
    assert d.offsets.grad is None or torch.isfinite(d.offsets.grad).all()
    wv, wt, info = ms.post_process_mesh((d.initial + d.offsets).detach(), d.geometry.tri, 200)
    assert torch.equal(fv, wv) and torch.equal(ft, wt) and info["reached"] and 199 <= ft.shape[0] <= 200
    assert fv.dtype == torch.float32 and ft.dtype == torch.int32 and not fv.requires_grad
    rr.invariants(fv.cpu().numpy(), ft.cpu().numpy().astype(np.int64))
    path = str(tmp_path / "final_mesh.obj")
    ms.write_obj(path, fv, ft)
    v2, t2 = template.load_obj(path)
    assert np.array_equal(_bits(v2.astype(np.float32)), _bits(fv)) and np.array_equal(t2, ft.cpu().numpy())
    d.step([0, 1])                                                      # and the deformation goes on


# ---- errors -------------------------------------------------------------------------------------------------------------------

def test_bad_calls_raise_value_errors_before_anything_is_written(monkeypatch):
    from garmentdreamer_amd import mesh_connectivity as mc, mesh_remesh as mr
    ms = _ms()
    launched = []
    real_ms, real_mr, real_mc = ms.launch, mr.launch, mc.launch
    monkeypatch.setattr(ms, "launch", lambda name, *a: (launched.append(name), real_ms(name, *a))[1])
    monkeypatch.setattr(mr, "launch", lambda name, *a: (launched.append(name), real_mr(name, *a))[1])
    monkeypatch.setattr(mc, "launch", lambda name, *a: (launched.append(name), real_mc(name, *a))[1])
    v, tri = _gpu_mesh(*sr.mesh("quad"))
    fan_v = _dev(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1]], dtype=np.float32))
    fan = _dev(np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], dtype=np.int32))                 # three faces on edge (0, 1)
    cases = [("no CPU path", lambda: ms.decimate_quadric(v.cpu(), tri, 1)),
             ("no CPU path", lambda: ms.decimate_quadric(v, tri.cpu(), 1)),
             ("no CPU path", lambda: ms.taubin_smooth(v.cpu(), tri)),
             ("no CPU path", lambda: ms.post_process_mesh(v, tri.cpu())),
             ("non-manifold", lambda: ms.decimate_quadric(fan_v, fan, 1)),
             ("non-manifold", lambda: ms.taubin_smooth(fan_v, fan)),
             ("non-manifold", lambda: ms.post_process_mesh(fan_v, fan, 1)),
             ("out of range", lambda: ms.decimate_quadric(v, _dev(np.array([[0, 1, 4]], dtype=np.int32)), 0)),
             ("out of range", lambda: ms.decimate_quadric(v, _dev(np.array([[0, 1, -1]], dtype=np.int64)), 0)),
             ("twice", lambda: ms.decimate_quadric(v, _dev(np.array([[0, 1, 1]], dtype=np.int32)), 0)),
             ("target_faces must be >= 0", lambda: ms.decimate_quadric(v, tri, -1)),
             ("passes must be >= 1", lambda: ms.decimate_quadric(v, tri, 1, passes=0))]
    for match, call in cases:
        with pytest.raises(ValueError, match=match) as e:
            call()
        assert "mesh_simplify." in str(e.value)
    print("entries launched:", sorted(set(launched)))
    assert set(launched) == {"gd_mesh_remesh_keys", "gd_mesh_remesh_heads", "gd_mesh_remesh_scan"}   # they write scratch only
    ov, ot, info = ms.decimate_quadric(v, _dev(np.zeros((0, 3), dtype=np.int32)), 0)
    assert ov.shape == v.shape and ot.shape == (0, 3) and info["reached"]
