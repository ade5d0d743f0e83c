"""The definition of include/gd_texture_sorted.h in float32 numpy on the CPU, twice: the REFERENCE of the sorted grid
gradient's tests.  Indices and weights are ``tests/texture_reference._cells``'s (the encoding's own statement).

  * ``encode_backward_sorted(x, denc, lay, mask, base)``          vectorised per level: ``np.add.at`` over the items in
    (n, i) order (``ufunc.at`` is unbuffered: it adds one item after the other in the order given), then ``base + s``
  * ``encode_backward_sorted_looped(...)``                        the same with plain Python loops over level, point, corner

Per entry with at least one item: ``s = +0``; ``s = s + weight_i * denc[n][l F + f]`` over its items in ascending (n, i), the
product rounded on its own; ``dgrid = base + s``.  An entry with no item keeps ``base``'s bits."""
import numpy as np
import torch

from tests import texture_reference as tref

F = tref.FEATURES


def _level_items(x, lay, l, mask):
    """(ok bool [N], idx int64 [N,8], weight float32 [N,8]) of level ``l``"""
    u, ok = tref._unit(x, torch.float32, mask)
    cells = tref._cells(u, lay, l)
    idx = np.stack([c[0].numpy() for c in cells], axis=1)
    wt = np.stack([c[1].numpy() for c in cells], axis=1)
    assert wt.dtype == np.float32
    return ok.numpy(), idx, wt


def _start(lay, denc, base):
    total = int(lay["offset"][-1])
    d = denc.detach().numpy()
    assert d.dtype == np.float32 and d.shape[1] == lay["num_levels"] * F
    out = np.zeros(total * F, dtype=np.float32) if base is None else base.detach().numpy().copy()
    assert out.dtype == np.float32 and out.shape == (total * F,)
    return d, out.reshape(total, F)


def encode_backward_sorted(x, denc, lay, mask=None, base=None):
    """dgrid float32 [offset_L F]: ``base`` (zeros if not given) plus the definition's sums"""
    d, out = _start(lay, denc, base)
    for l in range(lay["num_levels"]):
        ok, idx, wt = _level_items(x, lay, l, mask)
        size, off = int(lay["size"][l]), int(lay["offset"][l])
        e = idx[ok].reshape(-1)                                              # items in (n, i) order
        c = (wt[ok][:, :, None] * d[ok][:, None, F * l:F * (l + 1)]).reshape(-1, F)
        assert c.dtype == np.float32
        s = np.zeros((size, F), dtype=np.float32)
        np.add.at(s, e, c)
        touched = np.bincount(e, minlength=size) > 0
        out[off:off + size][touched] = out[off:off + size][touched] + s[touched]
    return torch.from_numpy(out.reshape(-1))


def encode_backward_sorted_looped(x, denc, lay, mask=None, base=None):
    d, out = _start(lay, denc, base)
    for l in range(lay["num_levels"]):
        ok, idx, wt = _level_items(x, lay, l, mask)
        size, off = int(lay["size"][l]), int(lay["offset"][l])
        s = np.zeros((size, F), dtype=np.float32)
        touched = np.zeros(size, dtype=bool)
        for n in range(x.shape[0]):
            if not ok[n]:
                continue
            for i in range(8):
                e = int(idx[n, i])
                for f in range(F):
                    c = np.float32(wt[n, i] * d[n, F * l + f])
                    s[e, f] = np.float32(s[e, f] + c)
                touched[e] = True
        for e in np.flatnonzero(touched):
            for f in range(F):
                out[off + e, f] = np.float32(out[off + e, f] + s[e, f])
    return torch.from_numpy(out.reshape(-1))


def touched(x, lay, mask=None):
    """bool [offset_L F]: the floats of the entries that have at least one item (a zero weight is an item too)"""
    out = np.zeros((int(lay["offset"][-1]), F), dtype=bool)
    for l in range(lay["num_levels"]):
        ok, idx, _ = _level_items(x, lay, l, mask)
        out[int(lay["offset"][l]) + idx[ok].reshape(-1)] = True
    return torch.from_numpy(out.reshape(-1))


def bits_equal(a, b):
    """the same float32 bits everywhere (the sign of a zero included)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def prefilled(n, seed=0):
    """float32 [n]: uniform in [-1, 1] with a -0.0 every fifth element and a +0.0 every seventh"""
    v = np.random.RandomState(seed).uniform(-1, 1, size=n).astype(np.float32)
    v[3::7] = 0.0
    v[1::5] = -0.0
    return torch.from_numpy(v)


LAYOUTS = {
    "enc4": dict(num_levels=4, base_resolution=3, per_level_scale=2.0, log2_hashmap_size=8),
    "fused16": dict(num_levels=16, base_resolution=2, per_level_scale=1.3, log2_hashmap_size=10),
    "res1": dict(num_levels=4, base_resolution=1, per_level_scale=2.0, log2_hashmap_size=8),   # level 0: res = 1
}


def mask_of(n):
    m = torch.ones(n, dtype=torch.uint8)
    m[4::7] = 0
    return m


def problem(name, n):
    """(lay, x [n,3] with the special rows, mask, denc, base) of the test plan"""
    lay = tref.layout(**LAYOUTS[name])
    x = tref.sample_points(n, seed=n + 2)
    denc = torch.from_numpy(np.random.RandomState(n).uniform(-1, 1, size=(n, lay["num_levels"] * F)).astype(np.float32))
    return lay, x, mask_of(n), denc, prefilled(int(lay["offset"][-1]) * F, seed=n + 5)
