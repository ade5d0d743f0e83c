"""CPU-side checks of the one error path of ``libgd_raster.so``'s binding (garmentdreamer_amd/_native.py): every entry
has an error channel that the library exports, and ``checked`` raises with that channel's own text.  No GPU is touched:
every failing call below is refused by the argument validation, before any HIP call."""
import pytest


def _tables(_native):
    return (_native.SIGNATURES, _native.SCENE_SIGNATURES, _native.MESH_SIGNATURES, _native.MESH_DEFORM_SIGNATURES,
            _native.MESH_GEOMETRY_SIGNATURES, _native.TEXTURE_SIGNATURES, _native.BAKE_SIGNATURES)


def test_every_entry_has_a_bound_error_channel():
    from garmentdreamer_amd import _native
    L = _native.lib()
    bound = set().union(*_tables(_native))
    assert len(bound) == sum(len(t) for t in _tables(_native))          # no symbol in two tables
    channels = set()
    for name in sorted(bound):
        channel = _native.error_channel(name)
        assert channel in bound and channel.endswith("_last_error") and hasattr(L, channel), name
        assert isinstance(getattr(L, channel)(), bytes)
        channels.add(channel)
    assert channels == {"gd_raster_last_error", "gd_scene_last_error", "gd_scene_densify_last_error", "gd_mesh_last_error",
                        "gd_texture_last_error", "gd_bake_last_error"}
    # the longest prefix decides
    assert _native.error_channel("gd_scene_densify_plan") == "gd_scene_densify_last_error"
    assert _native.error_channel("gd_scene_dist2") == "gd_scene_last_error"
    assert _native.error_channel("gd_mesh_normals_forward") == "gd_mesh_last_error"
    with pytest.raises(KeyError):
        _native.error_channel("gd_nn_conv3x3_forward")


def test_checked_returns_a_result_that_is_not_negative():
    from garmentdreamer_amd import _native
    for ret in (0, 1, 12345):
        assert _native.checked("gd_raster_forward", ret) == ret
        assert _native.check(ret, "gd_raster_forward") == ret and _native.check_scene(ret, "gd_scene_dist2") == ret
    assert _native.checked("gd_scene_dist2", _native.lib().gd_scene_dist2(None, 0, None, None, None)) == 0


def _failing_calls(_native):
    """entry -> (call, a piece of the message it leaves in its own channel)"""
    from garmentdreamer_amd import texture_field as tf
    L = _native.lib()
    null_cb = _native.ALLOC_FN(lambda u, n: 0)
    forward = [None, null_cb, None, null_cb, None, null_cb, None, 10, 0, 1, None, 0, 64] + [None] * 5 + [1.0] + \
        [None] * 5 + [0.5, 0.5, 0] + [None] * 4 + [0]                    # width == 0
    x = 0x1000                                                           # non-null and never followed
    return {
        "gd_raster_forward": (lambda: L.gd_raster_forward(*forward), "positive"),
        "gd_scene_dist2": (lambda: L.gd_scene_dist2(None, -1, None, None, None), "P must be"),
        "gd_scene_densify_stats": (lambda: L.gd_scene_densify_stats(None, -1, *([None] * 5)), "densify_stats: P must be"),
        "gd_scene_densify_plan": (lambda: L.gd_scene_densify_plan(None, 0, None, None, None, None, 0.0, 0.0, 0.0, 0.0,
                                                                  None, None), "densify_plan: P must be"),
        "gd_mesh_rasterize": (lambda: L.gd_mesh_rasterize(None, 3, 1, 0, 8, None, None, None, None), "positive"),
        "gd_mesh_visible_vertices": (lambda: L.gd_mesh_visible_vertices(None, 3, 1, 64, None, None, None), "null"),
        "gd_mesh_normals_forward": (lambda: L.gd_mesh_normals_forward(None, -1, 1, *([None] * 7)), ""),
        "gd_texture_encode_forward": (lambda: L.gd_texture_encode_forward(None, -1, x, None, x, tf.grid_layout(
            16, 2, 1.3, 10).struct(), x), "N must"),
        "gd_bake_pad_index": (lambda: L.gd_bake_pad_index(None, 8, 8, 4, None, x), "null"),
    }


def test_checked_raises_with_the_text_of_the_entrys_own_channel():
    from garmentdreamer_amd import _native
    L = _native.lib()
    calls = _failing_calls(_native)
    assert {_native.error_channel(n) for n in calls} == {_native.error_channel(n) for t in _tables(_native) for n in t}
    for name, (call, piece) in calls.items():
        ret = call()
        assert ret < 0, name
        text = getattr(L, _native.error_channel(name))().decode()
        assert text and piece in text, (name, text)
        with pytest.raises(RuntimeError) as info:
            _native.checked(name, ret)
        assert str(info.value) == f"{name} failed ({ret}): {text}"       # the entry's name, the code, the channel's text
        # the text is this channel's alone: every other channel holds something else
        others = {_native.error_channel(n) for n in calls} - {_native.error_channel(name)}
        assert all(getattr(L, c)().decode() != text for c in others), name
    # the older helpers are the same path with the channel named by the caller
    ret = calls["gd_raster_forward"][0]()
    with pytest.raises(RuntimeError, match=r"gd_raster_forward failed \(-1\): .*positive"):
        _native.check(ret, "gd_raster_forward")
    ret = calls["gd_scene_densify_plan"][0]()
    with pytest.raises(RuntimeError, match=r"densify failed \(-1\): densify_plan: P must be"):
        _native.check_scene(ret, "densify", "gd_scene_densify_last_error")
