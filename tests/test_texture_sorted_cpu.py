"""CPU-side checks of the sorted grid gradient (include/gd_texture_sorted.h): the REFERENCE
(tests/texture_sorted_reference.py) is pinned itself, its vectorised form bit for bit against the plain loops and, as a
float32 sum, against the float64 gradient; the header's entries are exported, bound in a table of their own and validate
their arguments without a GPU; the scratch query keeps its cap."""
import os
import re

import numpy as np
import pytest
import torch

from tests import texture_reference as tref
from tests import texture_sorted_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 63, 64, 65, 257)


def _rel(got, want64):
    return float((got.double() - want64).abs().max() / want64.abs().max())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(sref.LAYOUTS))
def test_reference_forms_bit_equal(name, n):
    lay, x, mask, denc, base = sref.problem(name, n)
    for m in (mask, None):
        for b in (base, None):
            vec = sref.encode_backward_sorted(x, denc, lay, m, b)
            assert vec.dtype == torch.float32
            assert sref.bits_equal(vec, sref.encode_backward_sorted_looped(x, denc, lay, m, b)), (name, n)
    # entries without an item keep the bits of the pre-filled buffer, -0.0 included; the others moved
    got = sref.encode_backward_sorted(x, denc, lay, mask, base)
    untouched = ~sref.touched(x, lay, mask)
    assert not (tref.encode_backward(x, denc, lay, mask)[untouched] != 0).any()
    if n > 1:
        assert untouched.any() and (~untouched).any()
    same = got.view(torch.int32) == base.view(torch.int32)
    assert bool(same[untouched].all())
    assert (base[untouched].view(torch.int32) == np.int32(-2 ** 31)).any()      # a -0.0 among them


def test_shared_entries_of_one_point_are_ordered_by_corner():
    """res = 1: corners 1, 2, 4 of every point share entry 1 and corners 3, 5, 6 entry 2"""
    lay = tref.layout(**sref.LAYOUTS["res1"])
    assert int(lay["res"][0]) == 1 and int(lay["size"][0]) == 8 and bool(lay["dense"][0])
    u = (tref.sample_points(40, seed=1)[:1] + 1) * 0.5
    idx = [int(c[0][0]) for c in tref._cells(u, lay, 0)]
    assert idx == [0, 1, 1, 2, 1, 2, 2, 3]


@pytest.mark.parametrize("name", sorted(sref.LAYOUTS))
def test_float32_sum_is_as_close_to_float64_as_the_scatter_reference(name):
    """the sequential float32 sum against the float64 gradient, by the project's measure (tests/test_texture_field_gpu.py):
    ``max|g - g64| / max|g64|`` within FOUR times the largest distance of the float32 ``tref.encode_backward`` over the three
    orders of the points (shuffled, ascending, descending).  One float32 sum is a sample of the rounding, another order
    another sample; without the factor the comparison of two samples fails by chance (enc4: 5.43e-7 against 5.37e-7)."""
    n = 257
    lay, x, mask, denc, _ = sref.problem(name, n)
    want = tref.encode_backward(x, denc.double(), lay, mask)
    own = 0.0
    for perm in (torch.from_numpy(np.random.RandomState(11).permutation(n)), torch.arange(n), torch.arange(n).flip(0)):
        own = max(own, _rel(tref.encode_backward(x[perm], denc[perm], lay, mask[perm]), want))
    err = _rel(sref.encode_backward_sorted(x, denc, lay, mask), want)
    print(f"{name}: sorted float32 {err:.3g}, float32 scatter reference {own:.3g}")
    assert err <= 4 * own, (name, err, own)


def _declared():
    text = open(os.path.join(ROOT, "include", "gd_texture_sorted.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gd_texture_[a-z0-9_]+)\s*\(", text)))


def test_sorted_symbols_declared_exported_and_bound():
    from garmentdreamer_amd import _native
    declared = _declared()
    L = _native.lib()
    assert declared == ["gd_texture_encode_backward_sorted", "gd_texture_field_backward_sorted",
                        "gd_texture_sorted_scratch_bytes"]
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/gd_texture_sorted.h but not exported"
        assert getattr(L, name).argtypes == _native.TEXTURE_SORTED_SIGNATURES[name][1]          # lib() bound the table
        assert _native.error_channel(name) == "gd_texture_last_error"
    assert sorted(_native.TEXTURE_SORTED_SIGNATURES) == declared
    others = set(_native.SIGNATURES) | set(_native.SCENE_SIGNATURES) | set(_native.MESH_SIGNATURES) \
        | set(_native.MESH_DEFORM_SIGNATURES) | set(_native.MESH_GEOMETRY_SIGNATURES) | set(_native.TEXTURE_SIGNATURES) \
        | set(_native.BAKE_SIGNATURES)
    assert not set(declared) & others


def _entries(L):
    """name -> (call(N, layout, pointers), number of pointers); the pointers in the order of the header, mask second"""
    return {
        "encode backward sorted": (lambda N, s, p: L.gd_texture_encode_backward_sorted(None, N, p[0], p[1], p[2], s, *p[3:]), 5),
        "field backward sorted": (lambda N, s, p: L.gd_texture_field_backward_sorted(None, N, p[0], p[1], p[2], s, *p[3:]), 17),
    }


def test_entries_validate_their_arguments():
    """-1 and a message before any device work (no GPU is touched: the stream is never used, no pointer is followed)"""
    from garmentdreamer_amd import _native
    from garmentdreamer_amd import texture_field as tf
    L = _native.lib()
    err = L.gd_texture_last_error
    lay = tf.grid_layout(16, 2, 1.3, 10)
    x = 0x1000                                     # non-null, 16-byte aligned, never followed
    for name, (call, nptr) in _entries(L).items():
        good = [x] * nptr
        assert call(0, lay.struct(), good) == 0, name                      # N == 0: nothing to do, nothing launched
        for N in (-1, -(1 << 31)):
            assert call(N, lay.struct(), good) == -1 and name.encode() in err() and b"N must" in err(), name
        assert call((1 << 24) + 1, lay.struct(), good) == -1, name         # beyond the sorted path's limit
        assert name.encode() in err() and b"2^24" in err() and b"atomic path" in err() and b"split" in err(), err()
        for hole in range(nptr):
            args = list(good)
            args[hole] = None
            if hole == 1:                                                  # the mask may be null; N = 0 keeps it a dry run
                assert call(0, lay.struct(), args) == 0, name
                continue
            assert call(5, lay.struct(), args) == -1 and b"null" in err() and name.encode() in err(), (name, hole)

        def broken(edit):
            s = lay.struct()
            edit(s)
            return call(5, s, good)

        def set_levels(v):
            return lambda s: setattr(s, "num_levels", v)

        def set_item(field, i, v):
            return lambda s: getattr(s, field).__setitem__(i, v)

        for what, edit in (("L = 0", set_levels(0)), ("L = 17", set_levels(17)), ("L = -1", set_levels(-1)),
                           ("size = 0", set_item("size", 3, 0)), ("size < 0", set_item("size", 0, -8)),
                           ("res = 0", set_item("res", 2, 0)), ("res < 0", set_item("res", 15, -1)),
                           ("equal offsets", set_item("offset", 4, lay.struct().offset[3])),
                           ("decreasing offsets", set_item("offset", 9, 5)),
                           ("offset[0] != 0", set_item("offset", 0, 8)),
                           ("offsets that skip entries", set_item("offset", 16, lay.struct().offset[16] + 8))):
            assert broken(edit) == -1 and b"layout" in err() and name.encode() in err(), (name, what)
            s = lay.struct()
            edit(s)
            assert L.gd_texture_sorted_scratch_bytes(1000, s) == 0, what   # the query: 0 for a bad layout
    call, nptr = _entries(L)["field backward sorted"]
    short = tf.grid_layout(4, 3, 2.0, 8)                                   # the fused path needs L F = 32
    assert call(5, short.struct(), [x] * nptr) == -1 and b"32" in err() and b"field backward sorted" in err()
    args = [x] * nptr
    args[2] = x + 4                                                        # the grid is read as float2
    assert call(5, lay.struct(), args) == -1 and b"aligned" in err()
    args = [x] * nptr
    args[14] = x + 8                                                       # denc is written as float4
    assert call(5, lay.struct(), args) == -1 and b"denc" in err() and b"aligned" in err()


def test_scratch_query():
    from garmentdreamer_amd import _native
    from garmentdreamer_amd import texture_field as tf
    L = _native.lib()
    small, prod = tf.grid_layout(4, 3, 2.0, 8), tf.grid_layout()
    for lay in (small, prod):
        s = lay.struct()
        assert L.gd_texture_sorted_scratch_bytes(0, s) == 0 and L.gd_texture_sorted_scratch_bytes(-7, s) == 0
        sizes = [L.gd_texture_sorted_scratch_bytes(n, s) for n in (1, 2, 63, 64, 65, 257, 3001, 1 << 18, (1 << 18) + 1,
                                                                   1 << 20, 1 << 24, (1 << 24) + 1, 1 << 26)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    for n in (1, 1 << 18, 1 << 24):
        got = L.gd_texture_sorted_scratch_bytes(n, prod.struct())
        print(f"scratch at N = {n}: {got} bytes, cap {4096 * n + (64 << 20)}")
        assert 0 < got <= 4096 * n + (64 << 20)


def test_python_keywords_default_to_the_atomic_path():
    import inspect
    from garmentdreamer_amd import texture_field as tf
    assert inspect.signature(tf.encode).parameters["deterministic"].default is False
    assert inspect.signature(tf.field).parameters["deterministic"].default is False
    small = tf.grid_layout(16, 2, 1.3, 10)
    assert tf.HashGridEncoder.from_layout(small).deterministic is False
    assert tf.HashGridEncoder.from_layout(small, deterministic=True).deterministic is True
    assert tf.HashGridEncoder(log2_hashmap_size=4, num_levels=2).deterministic is False
    assert tf.HashGridEncoder(log2_hashmap_size=4, num_levels=2, deterministic=True).deterministic is True
    enc = tf.HashGridEncoder.from_layout(small)
    assert tf.TextureField(enc).encoder.deterministic is False             # None leaves the encoder's flag
    assert tf.TextureField(enc, deterministic=True).encoder.deterministic is True and enc.deterministic is True
    assert tf.TextureField(enc, deterministic=False).encoder.deterministic is False
