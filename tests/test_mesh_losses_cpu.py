"""CPU-side checks of the second stage's G-buffer losses: the entries of include/gd_mesh_losses.h are exported, bound and
validate their arguments without a GPU; the REFERENCE (tests/mesh_losses_reference.py) is pinned itself: its two forms
against each other, both dtypes against values the reference's own functions produced
(tests/golden/deformer_loss_pins.npz), and its float64 autograd gradients against central differences."""
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_losses_reference as lref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TERMS = ("enhanced", "plain", "hole")


def test_loss_symbols_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "gd_mesh_losses.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(gd_mesh_[a-z0-9_]+)\s*\(", text)))
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert declared == ["gd_mesh_gbuffer_losses_backward", "gd_mesh_gbuffer_losses_forward",
                        "gd_mesh_gbuffer_losses_scratch_bytes"]
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_mesh_losses.h but not exported"
    assert sorted(_native.MESH_LOSS_SIGNATURES) == declared
    assert not set(declared) & (set(_native.MESH_SIGNATURES) | set(_native.MESH_DEFORM_SIGNATURES)
                                | set(_native.MESH_GEOMETRY_SIGNATURES))
    assert all(_native.error_channel(name) == "gd_mesh_last_error" for name in declared)
    for name, value in (("ENHANCED", _native.MESH_LOSS_ENHANCED), ("PLAIN", _native.MESH_LOSS_PLAIN),
                        ("HOLE", _native.MESH_LOSS_HOLE), ("STATS_WORDS", _native.MESH_LOSS_STATS_WORDS)):
        assert re.search(rf"#define GD_MESH_LOSSES_{name} {value}\b", text), name


def test_scratch_query():
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert L.gd_mesh_gbuffer_losses_scratch_bytes(1024 * 1024) >= 4096 * 6 * 4      # six partials per 256 pixels
    assert L.gd_mesh_gbuffer_losses_scratch_bytes(1) >= 6 * 4
    assert L.gd_mesh_gbuffer_losses_scratch_bytes(0) == 0
    assert L.gd_mesh_gbuffer_losses_scratch_bytes(-7) == 0


def test_entries_validate_their_arguments():
    """-1 and a message before any device work (no GPU is touched: the stream is never used).  The pointers, in order:
    normal position mask | normal_rf position_rf mask_rf | target_normal target_mask | camera | then stats scratch
    (forward) or stats dloss dnormal dposition (backward)."""
    from garmentdreamer_amd import _native
    L = _native.lib()
    err = L.gd_mesh_last_error
    x = 0x1000                                     # a non-null pointer that is never followed
    eps = -0.1
    entries = ((L.gd_mesh_gbuffer_losses_forward, 2, b"gbuffer losses"),
               (L.gd_mesh_gbuffer_losses_backward, 4, b"gbuffer losses backward"))
    for fn, tail, label in entries:
        def call(H, W, terms, ptrs):
            return fn(None, H, W, terms, *ptrs[:9], eps, *ptrs[9:])
        full = [x] * (9 + tail)
        for H, W in ((0, 4), (4, 0), (-1, 4), (4, -2), (1 << 15, 1 << 15)):
            assert call(H, W, 7, full) == -1 and label in err(), (H, W)
        for terms in (0, 8, -1):
            assert call(4, 4, terms, full) == -1 and b"terms" in err(), terms
        assert call(4, 4, 7, [None] * (9 + tail)) == -1 and b"null" in err()
        for hole in range(9 + tail):               # each pointer on its own, every term enabled
            ptrs = list(full)
            ptrs[hole] = None
            assert call(4, 4, 7, ptrs) == -1 and b"null" in err() and label in err(), hole
        for terms, needed in ((4, (3, 4, 5)), (1, (6, 7)), (2, (6, 7))):     # HOLE needs the _rf side, the others the targets
            for hole in needed:
                ptrs = list(full)
                ptrs[hole] = None
                assert call(4, 4, terms, ptrs) == -1 and b"null" in err(), (terms, hole)


def test_ops_reject_cpu_tensors():
    from garmentdreamer_amd import mesh_losses as ml
    case = lref.tensors(lref.make_case(3, 4, 5), torch.float32)
    view = ml.View(case["T"], case["tmask"], case["R"], case["center"])
    g = {k: case[k] for k in ("normal", "position", "mask")}
    for call in (lambda: ml.normal_map_loss_enhanced([view], [g]), lambda: ml.normal_map_loss([view], [g]),
                 lambda: ml.hole_mask_loss([view], [g], [g]), lambda: ml.second_stage_losses([view], [g], [g])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()


# ---- the reference, pinned ------------------------------------------------------------------------------------------------

def _pins():
    z = np.load(os.path.join(ROOT, "tests", "golden", "deformer_loss_pins.npz"))
    return {name: {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")} for name in ("view0", "view1", "both")}


def test_the_two_forms_agree():
    """float64; both forms evaluate the same expression per pixel and differ in the order of sums and of a few products:
    some ulp of values of order 1, asserted at 1e-13 of the largest gradient."""
    for H, W, seed in ((9, 11, 101), (16, 16, 102), (5, 7, 3)):
        case = lref.make_case(H, W, seed)
        for term in TERMS:
            a = lref.gradients(case, torch.float64, lref.LOSSES[term])
            b = lref.gradients(case, torch.float64, lref.GATHER_LOSSES[term])
            assert abs(float(a[0]) - float(b[0])) <= 1e-13 * abs(float(a[0])) and float(a[0]) > 0, term
            for x, y in zip(a[1:], b[1:]):
                assert np.abs(x - y).max() <= 1e-13 * max(np.abs(x).max(), 1e-300), term
            assert np.abs(a[1]).max() > 0
            assert (np.abs(a[2]).max() > 0) == (term == "hole")


def test_the_generator_keeps_the_thresholds_out():
    for H, W, seed in ((1, 1, 1), (5, 7, 2), (16, 16, 102)):
        case = lref.make_case(H, W, seed)
        assert not lref._near_a_threshold(case).any()
        for k in ("mask", "mask_rf", "tmask"):
            m = case[k]
            assert ((m == 0) | ((m >= 0.05) & (m <= 1))).all()
        a, b = lref.selections(case, torch.float64), lref.selections(case, torch.float32)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        assert a["enhanced"].any() and a["plain"].any() and a["hole"].any()
    first, again = lref.make_case(5, 7, 2), lref.make_case(5, 7, 2)
    assert all(np.array_equal(first[k], again[k]) for k in lref.KEYS)


@pytest.mark.parametrize("form", ["masked sum", "gather"])
def test_both_dtypes_agree_with_the_golden_pins(form):
    """The pins are float32 results of the reference's own functions.  The float32 statement repeats their operations up to
    the order of sums (1e-5 of the largest value is dozens of float32 ulp of sums over some hundred pixels); the float64
    statement differs from them by float32 rounding, the same bound."""
    pins = _pins()
    fns = lref.LOSSES if form == "masked sum" else lref.GATHER_LOSSES
    means = {term: {torch.float32: 0.0, torch.float64: 0.0} for term in TERMS}
    for name in ("view0", "view1"):
        case = {k: pins[name][k] for k in lref.KEYS}
        for term in TERMS:
            want = [pins[name][f"{term}/{k}"] for k in ("loss", "dnormal", "dposition")]
            assert np.abs(want[1]).max() > 0
            assert (np.abs(want[2]).max() > 0) == (term == "hole")       # position: from the hole-mask loss and no other
            for dtype in (torch.float32, torch.float64):
                got = lref.gradients(case, dtype, fns[term])
                means[term][dtype] += float(got[0]) / 2
                for what, g, w in zip(("loss", "dnormal", "dposition"), got, want):
                    scale = np.abs(w).max()
                    err = np.abs(g - w).max()
                    print(name, term, dtype, what, "max |got - pin|", err, "of", scale)
                    assert err <= 1e-5 * scale, (name, term, dtype, what)
    for term in TERMS:                                                    # each loss is the mean over the views
        for dtype in (torch.float32, torch.float64):
            assert abs(means[term][dtype] - float(pins["both"][f"{term}/loss"])) <= 1e-5 * means[term][dtype]


def test_reference_autograd_gradients_agree_with_central_differences():
    """float64, enhanced and plain towards ``normal``; 1e-6 steps of quantities of order 1: truncation ~1e-12, rounding
    ~1e-16 |L| / 1e-6 ~ 1e-10 against gradients of ~1e-2, asserted at 1e-6 of the largest.  The generator keeps every
    threshold 1e-3 away, so no pixel changes sides within a step."""
    case = lref.make_case(5, 7, 7)
    h = 1e-6
    for term in ("enhanced", "plain"):
        fn = lref.LOSSES[term]
        _, grad, dpos = lref.gradients(case, torch.float64, fn)
        assert not dpos.any()
        base = {k: v.astype(np.float64) for k, v in case.items()}
        fd = np.zeros(grad.shape)
        for idx in np.ndindex(*grad.shape):
            vals = []
            for sgn in (1, -1):
                moved = dict(base)
                moved["normal"] = base["normal"].copy()
                moved["normal"][idx] += sgn * h
                vals.append(float(fn(lref.tensors(moved, torch.float64))))
            fd[idx] = (vals[0] - vals[1]) / (2 * h)
        err = np.abs(fd - grad).max() / np.abs(grad).max()
        print(term, "max |fd - autograd| / max |autograd|", err)
        assert np.abs(grad).max() > 0 and err <= 1e-6
