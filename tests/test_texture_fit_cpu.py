"""CPU-side checks of the texture fit (garmentdreamer_amd/texture_fit.py, include/gd_fit.h): the host camera of a captured
view against its closed form, the entries exported, bound and validating their arguments without a GPU, the two statements
of tests/fit_reference.py against each other on the buffers the GPU tests use, and what the Python layer refuses before it
touches a kernel."""
import os
import re

import numpy as np
import pytest
import torch

from tests import fit_reference as fref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0x1000                                     # a non-null, 16-byte aligned pointer that is never followed

# camera positions t of c2w; fit_pose looks from (t_y, t_z, t_x): the 2nd, 3rd and 4th lie in the planes x = 0, z = 0 and
# y = 0 of that permuted frame
CAMERAS = [(1.2, 0.7, 2.0), (2.0, 0.0, 1.0), (0.0, 1.5, 1.0), (1.0, 2.0, 0.0), (-0.8, -1.1, 0.6), (0.3, 2.5, -1.7)]


def _unit(x):
    return x / np.linalg.norm(x)


def _c2w(t, seed=0):
    """a camera-to-world matrix at ``t`` with some rotation: fit_pose reads the position alone"""
    q, _ = np.linalg.qr(np.random.RandomState(seed).normal(size=(3, 3)))
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = q, t
    return m


@pytest.mark.parametrize("t", CAMERAS)
def test_fit_pose_against_its_closed_form(t):
    from garmentdreamer_amd.texture_fit import fit_pose
    pose = fit_pose(_c2w(t))
    assert pose.dtype == np.float32 and pose.shape == (4, 4)
    position = np.array([t[1], t[2], t[0]], dtype=np.float64)
    forward = _unit(position)
    right = _unit(np.cross([0.0, 1.0, 0.0], forward))
    up = _unit(np.cross(forward, right))
    want = np.eye(4)
    want[:3, 0], want[:3, 1], want[:3, 2], want[:3, 3] = -right, up, forward, position
    assert np.abs(pose - want).max() <= 1e-6
    assert np.array_equal(pose, fit_pose(_c2w(t, seed=1)))            # the view's own rotation is not read
    R = pose[:3, :3].astype(np.float64)
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R) + 1.0) <= 1e-6      # a mirrored camera
    assert np.array_equal(pose[3], [0, 0, 0, 1])


def test_fit_pose_refuses_what_has_no_look_at():
    from garmentdreamer_amd.texture_fit import fit_pose
    with pytest.raises(ValueError, match="off the y axis"):
        fit_pose(_c2w((0.0, 0.0, 2.0)))                                # permuted: (0, 2, 0)
    with pytest.raises(ValueError, match=r"\[4,4\]"):
        fit_pose(np.eye(3))


def test_fit_projection_is_the_renderers_projection():
    from garmentdreamer_amd import mesh_render as mr
    from garmentdreamer_amd.texture_fit import fit_projection
    K = np.array([[810.0, 0.0, 500.5], [0.0, 790.0, 530.25], [0.0, 0.0, 1.0]])
    got = fit_projection(K, 1024, 1000)
    assert got.dtype == np.float32
    assert np.array_equal(got, mr.projection(810.0, 790.0, 500.5, 530.25, 1024, 1000))
    assert got[0, 0] == np.float32(2 * 810.0 / 1024) and got[1, 2] == np.float32(1 - 2 * 530.25 / 1000)
    with pytest.raises(ValueError, match=r"\[3,3\]"):
        fit_projection(np.eye(4), 8, 8)


# ---- the entries ---------------------------------------------------------------------------------------------------------------

def test_fit_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gd_fit.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gd_fit_[a-z0-9_]+)\s*\(", code)))
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert declared == ["gd_fit_loss_backward", "gd_fit_loss_forward", "gd_fit_loss_scratch_bytes"]
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_fit.h but not exported"
        assert getattr(L, name).argtypes == _native.FIT_SIGNATURES[name][1]
        assert _native.error_channel(name) == "gd_mesh_last_error"
    assert sorted(_native.FIT_SIGNATURES) == declared
    k = fref.header_constants()
    assert k == {"PIXELS_PER_LANE": _native.FIT_PIXELS_PER_LANE, "PIXELS_PER_PARTIAL": _native.FIT_PIXELS_PER_PARTIAL,
                 "FINAL_THREADS": _native.FIT_FINAL_THREADS, "STATS_WORDS": _native.FIT_STATS_WORDS}
    from garmentdreamer_amd import _build
    assert ("raster_fit.hip", ["-ffp-contract=off"]) in _build.RASTER_SOURCES


def test_scratch_query_and_chain_length():
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert L.gd_fit_loss_scratch_bytes(1024 * 1024) >= 4096 * 8 and L.gd_fit_loss_scratch_bytes(1) >= 8
    assert L.gd_fit_loss_scratch_bytes(257 * 256) >= 257 * 8
    assert L.gd_fit_loss_scratch_bytes(0) == 0 and L.gd_fit_loss_scratch_bytes(-7) == 0
    # 2 channels + 3 in the lane + 6 in the wave's tree + the final pass's thread + 8 in its tree
    assert fref.chain_length(1) == 20 and fref.chain_length(256 * 256) == 20 and fref.chain_length(257 * 256) == 21
    assert fref.chain_length(1024 * 1024) == 19 + 16


def test_entries_validate_their_arguments():
    """-1 and a message before any device work (the stream is never used).  Pointers of the forward: c_aa a_aa p_aa n_aa
    center rgb tmask bg | image cosinesview m stats scratch; of the backward: c_aa a_aa rgb bg m stats dloss dc_aa."""
    from garmentdreamer_amd import _native
    L = _native.lib()
    err = L.gd_mesh_last_error
    entries = ((L.gd_fit_loss_forward, 13, b"fit loss", (0, 1, 2, 3, 5, 6, 8, 9, 10, 12)),
               (L.gd_fit_loss_backward, 8, b"fit loss backward", (0, 1, 2, 4, 7)))
    for fn, pointers, label, images in entries:
        full = [X] * pointers
        for H, W in ((0, 4), (4, 0), (-1, 4), (4, -2), (1 << 15, 1 << 15)):
            assert fn(None, H, W, 1, *full) == -1 and label in err() and b"positive" in err(), (H, W)
        assert fn(None, 4, 4, 1, *([None] * pointers)) == -1 and b"null" in err()
        for hole in range(pointers):
            ptrs = list(full)
            ptrs[hole] = None
            assert fn(None, 4, 4, 0, *ptrs) == -1 and b"null" in err() and label in err(), hole
        for at in images:                                              # an image off a 16-byte boundary
            ptrs = list(full)
            ptrs[at] = X + 4
            assert fn(None, 4, 4, 1, *ptrs) == -1 and b"aligned" in err() and label in err(), at
    with pytest.raises(RuntimeError, match=r"gd_fit_loss_forward failed \(-1\): fit loss: H and W must be positive"):
        _native.checked("gd_fit_loss_forward", L.gd_fit_loss_forward(None, 0, 4, 1, *([X] * 13)))


# ---- the two statements ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flip", (True, False))
@pytest.mark.parametrize("name", list(fref.SHAPES))
def test_float32_statement_against_the_composition_in_float64(name, flip):
    H, W, seed = fref.SHAPES[name]
    case = fref.make_case(H, W, seed)
    s32, s64 = fref.statement32(case, flip), fref.statement64(case, flip, dloss=0.7)
    count = int(s64["m"].sum())
    assert count > 0 and s32["count"] == count
    # the seeding keeps the selection away from cos = 0 but for the pixels put there on purpose
    candidates, near = int(s64["candidates"].sum()), int(s64["near"].sum())
    print(f"{name} flip={flip}: {count} selected of {candidates} candidates, {near} with |cos| < 2^-20")
    assert near < 1e-3 * candidates
    assert not ((s32["m"] != 0) != s64["m"])[~s64["near"]].any()
    if H * W >= 35:                                                    # every branch is there
        c, a = case["c_aa"], case["a_aa"]
        assert (c < 0).any() and (c > 1).any() and (c == 0).any() and (c == 1).any()
        assert (a < 0).any() and (a == 0).any() and (a > 1).any() and (a == 1).any() and (case["tmask"] == 0).any()
        assert (~case["n_aa"].any(-1)).any() and (case["p_aa"] == case["center"]).all(-1).any()
    if H * W >= 4096:
        assert near == 2 and (s32["cosinesview"][s64["near"]] == 0).all()
    bound = (fref.chain_length(H * W) + 8) * fref.U * s64["loss"]
    print(f"loss {s32['loss']:.9g} float64 {s64['loss']:.17g} |difference| {abs(float(s32['loss']) - s64['loss']):.3e} "
          f"allowed {bound:.3e}")
    assert abs(float(s32["loss"]) - s64["loss"]) <= bound
    assert np.abs(s32["image"] - s64["image"]).max() <= 3 * fref.U * 1.5
    # some twenty roundings of half an ulp each between the buffers and the cosine, |cos| <= 1
    assert np.abs(s32["cosinesview"] - s64["cosinesview"]).max() <= 12 * fref.U
    dc = fref.backward32(case, s32, 0.7)
    same = (s32["m"] != 0) == s64["m"]
    allowed = 16 * fref.U * 2 * 0.7 / (3 * count)
    assert np.abs(dc - s64["dc_aa"])[same].max() <= allowed
    assert not dc[s32["m"] == 0].any() and not dc[(case["c_aa"] < 0) | (case["c_aa"] > 1)].any()
    if H * W >= 35:                                                    # the bounds are inclusive
        at_bound = ((case["c_aa"] == 0) | (case["c_aa"] == 1)) & (s32["m"] != 0)[..., None]
        assert at_bound.sum() >= 3 and (dc[at_bound] != 0).all() and (s64["dc_aa"][at_bound] != 0).all()


def test_an_empty_selection():
    case = fref.make_case(5, 7, 3)
    case["tmask"][:] = 0
    s32 = fref.statement32(case, True)
    assert s32["count"] == 0 and s32["loss"] == 0 and s32["sum"] == 0 and not fref.backward32(case, s32, 1.0).any()
    assert np.isnan(fref.statement64(case, True)["loss"])              # the one deviation: the reference's mean over nothing


# ---- what the Python layer refuses ---------------------------------------------------------------------------------------------

def _cpu_buffers(h=4, w=4):
    z3, z1 = torch.zeros(h, w, 3), torch.zeros(h, w)
    return (z3, z1, z3, z3, torch.zeros(3)), z3, z1


def test_argument_validation_without_a_gpu():
    from garmentdreamer_amd import texture_fit as fit
    buffers, rgb, mask = _cpu_buffers()
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit.fit_loss(buffers, rgb, mask)
    with pytest.raises(ValueError, match="c_aa, a_aa, p_aa, n_aa, center"):
        fit.fit_loss(buffers[:4], rgb, mask)
    with pytest.raises(ValueError, match="at least one view"):
        fit.fit_texture(None, [])
    with pytest.raises(RuntimeError, match="no CPU path"):
        fit.background(torch.ones(3), "cpu")
    with pytest.raises(ValueError, match="one number or three"):
        fit.background((1.0, 0.5), "cpu")
    assert torch.equal(fit.background(0.25, "cpu"), torch.full((3,), 0.25))
    from garmentdreamer_amd.texture_field import NeTFRenderer
    assert callable(NeTFRenderer.fit_texture_from_mesh)
    assert fit.FitView._fields == ("c2w", "K", "rgb", "mask")
    assert fit.FitBuffers._fields == ("c_aa", "a_aa", "p_aa", "n_aa", "center")
