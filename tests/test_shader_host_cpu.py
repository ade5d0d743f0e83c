"""CPU-side checks of the neural shader's host layer: the entries of include/gd_shader.h are exported, bound in
``_native.SHADER_SIGNATURES`` and validate their arguments without a GPU (the stream is never used: every failing call is
refused before any HIP call), and ``NeuralShader`` / ``mesh_losses.shading_loss`` refuse what they have no kernel for."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import mesh_losses_reference as lref
from tests import shader_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = 0x1000                                     # a non-null pointer that is never followed


def _declared():
    text = open(os.path.join(ROOT, "include", "gd_shader.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    entries = text[text.index('extern "C" {'):]                      # behind the inline functions
    return text, sorted(set(re.findall(r"\b(gd_shader_[a-z0-9_]+)\s*\(", entries)))


def test_shader_symbols_declared_exported_and_bound():
    from garmentdreamer_amd import _native
    text, declared = _declared()
    L = _native.lib()
    assert len(declared) == 13 and "gd_shader_forward_layer" in declared and "gd_shader_hash32" not in declared
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_shader.h but not exported"
        assert getattr(L, name).argtypes == _native.SHADER_SIGNATURES[name][1]           # lib() bound the table
        assert _native.error_channel(name) == "gd_mesh_last_error"
    assert sorted(_native.SHADER_SIGNATURES) == declared
    others = set(_native.SIGNATURES) | set(_native.SCENE_SIGNATURES) | set(_native.MESH_SIGNATURES) \
        | set(_native.MESH_DEFORM_SIGNATURES) | set(_native.MESH_GEOMETRY_SIGNATURES) | set(_native.MESH_LOSS_SIGNATURES) \
        | set(_native.TEXTURE_SIGNATURES) | set(_native.TEXTURE_SORTED_SIGNATURES) | set(_native.BAKE_SIGNATURES)
    assert not set(declared) & others and not any(name.endswith("_last_error") for name in declared)
    for name, value in (("LAYERS", _native.SHADER_LAYERS), ("TILE_ROWS", _native.SHADER_TILE_ROWS),
                        ("PACKED_ELEMS", _native.SHADER_PACKED_ELEMS), ("PARAM_ELEMS", _native.SHADER_PARAM_ELEMS)):
        assert re.search(rf"#define GD_SHADER_{name} {value}\b", text), name
    from garmentdreamer_amd import neural_shader as ns
    assert ns.LAYER_NAMES == sref.NAMES and ns.IN_FEATURES == sref.IN_FEATURES and ns.OUT_FEATURES == sref.OUT_FEATURES
    assert (ns.ACT_WIDTH, ns.DZ_WIDTH) == (1600, 1568) and ns.rows_of(1) == ns.rows_of(128) == 128 and ns.rows_of(129) == 256


def test_scratch_queries():
    from garmentdreamer_amd import _native
    L = _native.lib()
    assert L.gd_shader_select_scratch_bytes(1024 * 1024) >= 4096 * 2 * 4 and L.gd_shader_select_scratch_bytes(1) >= 8
    assert L.gd_shader_select_scratch_bytes(0) == 0 and L.gd_shader_select_scratch_bytes(-3) == 0
    one_slab = (256 * 256 + 256) * 4
    assert L.gd_shader_scratch_bytes(1) >= one_slab + 4 and L.gd_shader_scratch_bytes(128) == L.gd_shader_scratch_bytes(1)
    assert L.gd_shader_scratch_bytes(1 << 20) >= 64 * one_slab + 4096 * 4
    assert L.gd_shader_scratch_bytes(0) == 0 and L.gd_shader_scratch_bytes(-1) == 0 and L.gd_shader_scratch_bytes((1 << 24) + 1) == 0


# entry -> (the arguments behind the stream with every pointer set, the positions of its pointers that may be NULL there,
# the positions of H and W or of N, the position of capacity)
def _entries():
    cap = C.c_int64(100)
    f, u = C.c_float(0.5), C.c_uint32(0)
    return {
        "gd_shader_select": ([8, 8, X, X, X, X, X, f, u, u, cap, X, X, X], (), (0, 1), 10),
        "gd_shader_features": ([8, 8, X, X, X, cap, X, X, X], (), (0, 1), 5),
        "gd_shader_features_points": ([C.c_int64(50), X, X, X, cap, X, X], (), (0,), 4),
        "gd_shader_pack": ([X, X, X], (), (), None),
        "gd_shader_forward_layer": ([3, cap, X, X, X, X, X], (6,), (), 1),
        "gd_shader_backward_input_layer": ([3, cap, X, X, X, X, X, X], (6, 7), (), 1),
        "gd_shader_backward_weight_layer": ([3, cap, X, X, X, X, X], (), (), 1),
        "gd_shader_l1_forward": ([8, 8, cap, X, X, X, X, X, X], (), (0, 1), 2),
        "gd_shader_l1_backward": ([8, 8, cap, X, X, X, X, X, X, X], (9,), (0, 1), 2),
        "gd_shader_colour": ([C.c_int64(50), X, X], (), (0,), None),
        "gd_shader_features_backward": ([8, 8, X, X, cap, X, X, X, X, X, X], (), (0, 1), 4),
    }


def test_entries_validate_their_arguments():
    from garmentdreamer_amd import _native
    L = _native.lib()
    err = L.gd_mesh_last_error
    table = _entries()
    assert sorted(table) == sorted(n for n, (res, _) in _native.SHADER_SIGNATURES.items() if res is C.c_int)
    for name, (args, optional, sizes, capacity_at) in table.items():
        fn = getattr(L, name)
        pointers = [i for i, a in enumerate(args) if a is X]
        assert fn(None, *[None if i in pointers else a for i, a in enumerate(args)]) == -1 and b"null" in err(), name
        for hole in pointers:
            if hole not in optional:
                assert fn(None, *[None if i == hole else a for i, a in enumerate(args)]) == -1 and b"null" in err(), (name, hole)
        for at in sizes:
            for bad in (0, -1):
                value = C.c_int64(bad) if isinstance(args[at], C.c_int64) else bad
                assert fn(None, *[value if i == at else a for i, a in enumerate(args)]) == -1 and err(), (name, at, bad)
                assert b"positive" in err() or b"must be in" in err(), (name, err())
        if capacity_at is not None:
            for bad in (0, -5, (1 << 24) + 1):
                assert fn(None, *[C.c_int64(bad) if i == capacity_at else a for i, a in enumerate(args)]) == -1, (name, bad)
                assert b"capacity" in err(), (name, err())
    # the pointers a layer needs: logits for layer 7, dfeat for layer 0, dextra for layer 5
    cap = C.c_int64(100)
    assert L.gd_shader_forward_layer(None, 7, cap, X, X, X, X, None) == -1 and b"null" in err()
    assert L.gd_shader_backward_input_layer(None, 0, cap, X, X, X, X, None, X) == -1 and b"null" in err()
    assert L.gd_shader_backward_input_layer(None, 5, cap, X, X, X, X, X, None) == -1 and b"null" in err()
    for fn, tail in ((L.gd_shader_forward_layer, 5), (L.gd_shader_backward_input_layer, 6), (L.gd_shader_backward_weight_layer, 5)):
        for l in (-1, 8):
            assert fn(None, l, cap, *[X] * tail) == -1 and b"layer" in err()
    assert L.gd_shader_select(None, 1 << 15, 1 << 15, *[X] * 5, C.c_float(0.5), 0, 0, cap, X, X, X) == -1 and b"2^30" in err()
    assert L.gd_shader_select(None, 8, 8, *[X] * 5, C.c_float(-0.5), 0, 0, cap, X, X, X) == -1 and b"negative" in err()
    assert L.gd_shader_select(None, 8, 8, *[X] * 5, C.c_float(float("nan")), 0, 0, cap, X, X, X) == -1
    assert L.gd_shader_features_points(None, C.c_int64(101), X, X, X, cap, X, X) == -1 and b"N must be" in err()
    with pytest.raises(RuntimeError, match="gd_shader_pack failed.*null pointer"):
        _native.checked("gd_shader_pack", L.gd_shader_pack(None, None, None, None))


def test_the_python_layer_refuses_what_it_has_no_kernel_for():
    from garmentdreamer_amd import mesh_losses as ml
    from garmentdreamer_amd.neural_shader import NeuralShader
    view = ml.View(1, 2, 3, 4)                                          # four arguments still construct
    assert view.rgb is None and view._fields == ("normal", "mask", "R", "center", "rgb")
    assert ml.View(1, 2, 3, 4, 5).rgb == 5
    with pytest.raises(RuntimeError, match="no CPU path"):
        NeuralShader(device="cpu")
    for bad in ({"hidden_features_layers": 7}, {"hidden_features_size": 128}, {"fft_scale": 10}, {"activation": "tanh"},
                {"fourier_features": "gfft"}, {"last_activation": torch.nn.Tanh()}, {"mapping_size": 128}):
        with pytest.raises(ValueError, match="built for"):
            NeuralShader(device="cpu", **bad)
    with pytest.raises(TypeError, match="NeuralShader"):
        ml.shading_loss([view], [{}], torch.nn.Linear(3, 3))
    shader = object.__new__(NeuralShader)                               # no GPU here: the checks below come before any use
    shader._params = {}
    case = lref.tensors(lref.make_case(3, 4, 5), torch.float32)
    g = {"normal": case["normal"], "position": case["position"], "mask": case["mask"]}
    rgb = torch.rand(3, 4, 3)
    full = ml.View(case["T"], case["tmask"], case["R"], case["center"], rgb)
    with pytest.raises(ValueError, match="no rgb"):
        ml.shading_loss([ml.View(case["T"], case["tmask"], case["R"], case["center"])], [g], shader)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ml.shading_loss([full], [g], shader)
    with pytest.raises(ValueError, match=r"view.rgb must be \[H,W,3\]"):
        ml.shading_loss([full._replace(rgb=torch.rand(3, 4))], [g], shader)
    with pytest.raises(ValueError, match="one shape"):
        NeuralShader.__call__(shader, case["position"], case["normal"], case["normal"][:2])
    with pytest.raises(ValueError, match="one shape"):
        NeuralShader.__call__(shader, case["position"][..., :2], case["normal"][..., :2], case["normal"][..., :2])
    with pytest.raises(ValueError, match="one G-buffer per view"):
        ml.shading_loss([full], [g, g], shader)
    with pytest.raises(ValueError, match="negative"):
        ml.shading_loss([full], [g], shader, shading_percentage=-0.1)
    with pytest.raises(ValueError, match="32 bits"):
        ml.shading_loss([full], [g], shader, seed=-1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        NeuralShader.__call__(shader, case["position"], case["normal"], case["normal"])
