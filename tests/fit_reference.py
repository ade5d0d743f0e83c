"""The definitions of include/gd_fit.h stated twice on the CPU, plus the seeded generator of synthetic buffers.

  * ``statement32``   float32 numpy, every operation and every sum in the header's order: meant to be bit-comparable with the
                      kernels (numpy rounds each product and sum on its own, as the kernels built with -ffp-contract=off do)
  * ``statement64``   float64 torch, the reference's literal composition: clamp, composite, ``F.normalize``,
                      ``cosine_similarity``, the three masks, ``flipud`` and ``MSELoss`` over the boolean gather, with autograd

A case is a dict of float32 arrays: ``c_aa``, ``p_aa``, ``n_aa``, ``rgb`` [H,W,3], ``a_aa``, ``tmask`` [H,W], ``center``,
``bg`` [3]."""
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("c_aa", "a_aa", "p_aa", "n_aa", "center", "rgb", "tmask", "bg")
U = 2.0 ** -24
NEAR = 2.0 ** -20          # a float64 |cos| below this may fall on the other side of 0 in float32
# H, W, seed: one pixel; less than a wave; a multiple of 256; 35 partials with a ragged last one and a width that is no
# multiple of 4; 257 partials, so that thread 0 of the final pass adds two
SHAPES = {"1x1": (1, 1, 21), "5x7": (5, 7, 22), "64x64": (64, 64, 23), "67x131": (67, 131, 24), "257x256": (257, 256, 25)}


def header_constants():
    text = open(os.path.join(ROOT, "include", "gd_fit.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define GD_FIT_([A-Z_]+) (\d+)\b", text)}


def partials_of(npix):
    return -(-npix // header_constants()["PIXELS_PER_PARTIAL"])


def chain_length(npix):
    """D: the longest chain of additions a term of the sum passes through in the header's order: the three channels, the
    lane's pixels, the tree over the partial's lanes, the final pass's thread, its tree."""
    k = header_constants()
    lanes = k["PIXELS_PER_PARTIAL"] // k["PIXELS_PER_LANE"]
    return 2 + (k["PIXELS_PER_LANE"] - 1) + int(math.log2(lanes)) + -(-partials_of(npix) // k["FINAL_THREADS"]) \
        + int(math.log2(k["FINAL_THREADS"]))


# ---- float32, the header's order ---------------------------------------------------------------------------------------------

def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def _clamp01(x):
    return np.where(x < 0, np.float32(0), np.where(x > 1, np.float32(1), x)).astype(np.float32)


def _tree(x, width):
    """x [groups, width] -> [groups]: stride width / 2, ..., 1: x[l] += x[l + stride]"""
    x = x.copy()
    stride = width // 2
    while stride:
        x[:, :stride] = x[:, :stride] + x[:, stride:2 * stride]
        stride //= 2
    return x[:, 0]


def ordered_sum(e):
    """the header's sum of the per-pixel values ``e`` (float32 or int32, flat)"""
    k = header_constants()
    per_lane, per_partial, threads = k["PIXELS_PER_LANE"], k["PIXELS_PER_PARTIAL"], k["FINAL_THREADS"]
    partials = -(-e.size // per_partial)
    x = np.zeros(partials * per_partial, dtype=e.dtype)
    x[:e.size] = e
    x = x.reshape(partials, per_partial // per_lane, per_lane)
    q = x[..., 0]
    for j in range(1, per_lane):
        q = q + x[..., j]
    part = _tree(q, per_partial // per_lane)
    rounds = -(-partials // threads)
    y = np.zeros(rounds * threads, dtype=e.dtype)
    y[:partials] = part
    y = y.reshape(rounds, threads)
    acc = np.zeros(threads, dtype=e.dtype)
    for r in range(rounds):
        acc = acc + y[r]
    return _tree(acc[None], threads)[0]


def statement32(case, flip):
    """dict: image, cosinesview, m (uint8), r (image - target), a, count (int), sum, loss (float32)"""
    f = np.float32
    c_aa, a_aa, p_aa, n_aa = (case[k] for k in ("c_aa", "a_aa", "p_aa", "n_aa"))
    rgb, tmask = (case[k][::-1] if flip else case[k] for k in ("rgb", "tmask"))
    a = _clamp01(a_aa)
    u = f(1) - a
    image = a[..., None] * _clamp01(c_aa) + u[..., None] * case["bg"]
    d = p_aa - case["center"]
    d = d / np.maximum(np.sqrt(_dot(d, d)), f(1e-12))[..., None]
    cos = _dot(d, n_aa) / (np.maximum(np.sqrt(_dot(d, d)), f(1e-6)) * np.maximum(np.sqrt(_dot(n_aa, n_aa)), f(1e-6)))
    m = (a > 0) & (tmask > 0) & (cos <= 0)
    r = image - rgb
    e = np.where(m, _dot(r, r), f(0)).astype(f)
    count = int(ordered_sum(m.reshape(-1).astype(np.int32)))
    total = ordered_sum(e.reshape(-1))
    loss = total / (f(3) * f(count)) if count else f(0)
    assert all(x.dtype == f for x in (image, cos, r, e)) and np.asarray(total).dtype == f
    return {"image": image, "cosinesview": cos, "m": m.astype(np.uint8), "r": r, "a": a, "count": count, "sum": f(total),
            "loss": f(loss)}


def backward32(case, s, dloss):
    """dc_aa of the header from ``s = statement32(case, flip)``"""
    f = np.float32
    g = (f(2) * f(dloss)) / (f(3) * f(s["count"])) if s["count"] else f(0)
    keep = (s["m"] != 0)[..., None] & (case["c_aa"] >= 0) & (case["c_aa"] <= 1)
    return np.where(keep, (g * s["r"]) * s["a"][..., None], f(0)).astype(f)


# ---- float64, the reference's composition -------------------------------------------------------------------------------------

def composition(c_aa, a_aa, p_aa, n_aa, center, rgb, tmask, bg, flip=True):
    """(loss, image, cosinesview, mask) as Renderer.render's tail and fit_texture_from_mesh state them, in the tensors'
    dtype and on their device; the loss of an empty selection is NaN, as the reference's is"""
    alpha = a_aa.clamp(0, 1)[..., None]
    image = alpha * c_aa.clamp(0, 1) + (1 - alpha) * bg
    with torch.no_grad():
        view_direction = F.normalize(p_aa - center, dim=-1)
        cosines = F.cosine_similarity(view_direction, n_aa, dim=-1, eps=1e-6)
    if flip:
        rgb, tmask = torch.flipud(rgb), torch.flipud(tmask)
    mask = (alpha[..., 0] > 0) & (tmask > 0) & (cosines <= 0)
    return torch.nn.MSELoss()(image[mask], rgb[mask]), image, cosines, mask


def statement64(case, flip, dloss=1.0):
    """dict of numpy float64: loss, dc_aa, image, cosinesview, m (bool), near (bool: candidates with |cos| < 2^-20),
    candidates (bool: a > 0 and target mask > 0)"""
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).double() for k in KEYS}
    t["c_aa"].requires_grad_(True)
    loss, image, cos, mask = composition(*[t[k] for k in KEYS], flip=flip)
    dc = np.zeros(case["c_aa"].shape)
    if bool(mask.any()):
        loss.backward(torch.tensor(float(dloss), dtype=torch.float64))
        dc = t["c_aa"].grad.numpy()
    tm = case["tmask"][::-1] if flip else case["tmask"]
    candidates = (case["a_aa"] > 0) & (tm > 0)
    return {"loss": float(loss.detach()), "dc_aa": dc, "image": image.detach().numpy(), "cosinesview": cos.numpy(),
            "m": mask.numpy(), "candidates": candidates, "near": candidates & (np.abs(cos.numpy()) < NEAR)}


# ---- synthetic buffers --------------------------------------------------------------------------------------------------------

def make_case(H, W, seed):
    """Seeded buffers that hold every branch of the head (from 5 x 7 on): ``c_aa`` below 0, above 1 and exactly 0 and 1 (on
    selected pixels: the clamp passes a gradient at its bounds), ``a_aa`` <= 0 (exactly 0 too) and > 1 (exactly 1 too), a
    zero ``n_aa``, ``p_aa == center``, target masks of exactly 0.
    The zero normal and the position at the centre give a cosine of exactly 0; they sit on pixels outside the selection's
    candidates (target mask 0, alpha <= 0, also upside down), and from 64 x 64 on one of each sits inside as well."""
    rng = np.random.RandomState(seed)
    n = H * W
    center = np.array([0.3, -0.2, 3.0]) + 0.1 * rng.normal(size=3)
    p = rng.uniform(-0.5, 0.5, (n, 3))
    nrm = rng.normal(size=(n, 3))
    nrm *= (rng.uniform(0.6, 1.0, (n, 1)) / np.linalg.norm(nrm, axis=-1, keepdims=True))
    c = rng.uniform(-0.3, 1.3, (n, 3))
    a = rng.uniform(-0.3, 1.4, n)
    tmask = rng.uniform(0.05, 1.0, n) * (rng.uniform(size=n) >= 0.2)
    rgb = rng.uniform(0.0, 1.0, (n, 3))
    if n == 1:
        a[0], tmask[0], c[0] = 0.7, 0.5, (0.4, -0.1, 1.2)
        nrm[0] = center - p[0]                                  # faces the camera: cos = -1
    else:
        rows = lambda i: (i, (H - 1 - i // W) * W + i % W)     # a pixel and the one whose targets it reads when flipped
        free = list(rng.permutation(n))
        for channel, value in ((0, 0.0), (1, 1.0), (2, 0.0)):   # the clamp's bounds, on pixels that are selected
            i = free.pop()
            c[i, channel], a[i], nrm[i] = value, 0.7, center - p[i]
            tmask[list(rows(i))] = 0.5
        a[free.pop()], a[free.pop()] = 0.0, 1.0
        i = free.pop()
        nrm[i] = 0.0
        tmask[list(rows(i))] = 0.0
        i = free.pop()
        p[i], a[i] = center, -0.1
        if n >= 4096:
            i, j = free.pop(), free.pop()
            nrm[i], p[j] = 0.0, center
            for k in (i, j):
                a[k] = 0.7
                tmask[list(rows(k))] = 0.5
    shape = lambda x: np.ascontiguousarray(x.astype(np.float32).reshape((H, W) + x.shape[1:]))
    case = {"c_aa": shape(c), "a_aa": shape(a), "p_aa": shape(p), "n_aa": shape(nrm), "rgb": shape(rgb),
            "tmask": shape(tmask), "center": center.astype(np.float32), "bg": np.array([1.0, 0.9, 0.75], np.float32)}
    if n > 1:                                                   # p == center in float32, exactly
        case["p_aa"].reshape(n, 3)[np.all(p == center, axis=-1)] = case["center"]
    return case
