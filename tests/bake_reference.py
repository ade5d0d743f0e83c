"""numpy statement of the texture bake's padding (include/gd_bake.h): the checker of tests/test_texture_bake_*.py.  The
definition twice, with plain loops over ALL covered texels and vectorised; the scipy / scikit-learn formulation that
kiui's ``uv_padding(..., backend='knn')`` is understood to be; the 8-bit resolve; the coverage of an atlas at texel
centres by the rasterizer's rule (include/gd_mesh.h), in integers.  Test infrastructure: never imported by the package."""
import numpy as np


def pad_index_loops(mask, p):
    """src int32 [H,W], the header's definition word for word: every covered texel is a candidate, in row-major order."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    covered = [(r, c) for r in range(H) for c in range(W) if mask[r, c]]
    src = np.full((H, W), -1, dtype=np.int32)
    for r in range(H):
        for c in range(W):
            if mask[r, c]:
                src[r, c] = r * W + c
                continue
            best, arg, witness = None, -1, False
            for rr, cc in covered:
                if abs(r - rr) + abs(c - cc) <= p:
                    witness = True
                d2 = (r - rr) ** 2 + (c - cc) ** 2
                if best is None or d2 < best:          # strict: the first (lowest index) of equals stays
                    best, arg = d2, rr * W + cc
            if witness:
                src[r, c] = arg
    return src


def pad_index(mask, p, with_ties=False):
    """The same, vectorised (the uncovered texels in chunks against ALL covered texels): argmin returns the first
    minimum, and the candidates are listed in row-major order.  ``with_ties``: also bool [H,W], true where an uncovered
    texel that gets a source has more than one nearest covered texel."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    src = np.full(H * W, -1, dtype=np.int32)
    ties = np.zeros(H * W, dtype=bool)
    rr, cc = (a.astype(np.int32) for a in np.nonzero(mask))           # row-major order
    src[rr * W + cc] = rr * W + cc
    todo = np.flatnonzero(~mask.ravel())
    if rr.size:
        for a in range(0, todo.size, 1024):
            t = todo[a:a + 1024]
            dr = (t // W).astype(np.int32)[:, None] - rr[None, :]
            dc = (t % W).astype(np.int32)[:, None] - cc[None, :]
            d2 = dr * dr + dc * dc
            arg = np.argmin(d2, axis=1)
            fill = (np.abs(dr) + np.abs(dc)).min(axis=1) <= p
            src[t[fill]] = (rr[arg] * W + cc[arg])[fill]
            ties[t] = fill & ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1)
    src = src.reshape(H, W)
    return (src, ties.reshape(H, W)) if with_ties else src


def knn_formulation(image, mask, p):
    """(region bool [H,W], padded image): the region to fill is ``binary_dilation(mask, iterations=p)`` with scipy's default
    (4-connected) element minus the mask; every texel of it takes the colour of its one nearest neighbour, by a KD-tree,
    among the mask's two outer layers (the mask minus its erosion by two iterations)."""
    from scipy.ndimage import binary_dilation, binary_erosion
    from sklearn.neighbors import NearestNeighbors
    mask = np.asarray(mask) != 0
    out = np.array(image, copy=True)
    region = np.zeros_like(mask)
    if p > 0 and mask.any():                               # iterations=0 would mean "until nothing changes"
        region = binary_dilation(mask, iterations=p) & ~mask
    if region.any():
        search = mask & ~binary_erosion(mask, iterations=2)
        search_coords = np.stack(np.nonzero(search), axis=-1)
        fill_coords = np.stack(np.nonzero(region), axis=-1)
        knn = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(search_coords)
        _, found = knn.kneighbors(fill_coords)
        out[tuple(fill_coords.T)] = image[tuple(search_coords[found[:, 0]].T)]
    return region, out


def resolve_u8(image, src):
    """uint8 [H,W,C] of the header's RESOLVE, in float32 numpy"""
    image = np.asarray(image, dtype=np.float32)
    H, W, C = image.shape
    flat = image.reshape(H * W, C)
    s = np.asarray(src).reshape(-1).astype(np.int64)
    follow = (s >= 0) & (s < H * W)
    x = flat[np.where(follow, s, 0)]
    with np.errstate(invalid="ignore"):
        x = np.where(x > 0, np.where(x < 1, x, np.float32(1)), np.float32(0)).astype(np.float32)   # NaN -> 0
        q = (x * np.float32(255.0)).astype(np.int32).astype(np.uint8)
    return np.where(follow[:, None], q, np.uint8(0)).astype(np.uint8).reshape(H, W, C)


def chart_coverage(vt, ft, H, W):
    """bool [H,W]: texel centres covered by some triangle of the atlas, by the rasterizer's rule (include/gd_mesh.h): edge
    functions in integers (1/256 texel, as the rasterizer snaps), a centre ON an edge belongs to the triangle iff the
    edge, with the triangle oriented to positive area, has dY > 0 or dY == 0 and dX < 0."""
    vt = np.asarray(vt, dtype=np.float64)
    ft = np.asarray(ft, dtype=np.int64)
    X = np.rint(vt[:, 0] * 256 * W).astype(np.int64)[ft]          # [F,3]
    Y = np.rint(vt[:, 1] * 256 * H).astype(np.int64)[ft]
    Px = (256 * np.arange(W, dtype=np.int64) + 128)[None, :]
    Py = (256 * np.arange(H, dtype=np.int64) + 128)[:, None]
    cover = np.zeros((H, W), dtype=bool)
    for t in range(ft.shape[0]):
        x, y = X[t], Y[t]
        A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if A == 0:
            continue
        sign = 1 if A > 0 else -1
        inside = np.ones((H, W), dtype=bool)
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            dX, dY = sign * (x[k] - x[j]), sign * (y[k] - y[j])
            e = dX * (Py - y[j]) - dY * (Px - x[j])
            inside &= (e > 0) | ((e == 0) & ((dY > 0) or (dY == 0 and dX < 0)))
        cover |= inside
    return cover


def blob_mask(H, W, seed, blobs=5):
    """a few random discs and a few single texels"""
    rng = np.random.RandomState(seed)
    r, c = np.mgrid[0:H, 0:W]
    mask = np.zeros((H, W), dtype=bool)
    for _ in range(blobs):
        cr, cc, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1.0, 5.0)
        mask |= (r - cr) ** 2 + (c - cc) ** 2 <= rad * rad
    mask[rng.randint(0, H, 4), rng.randint(0, W, 4)] = True
    return mask


# (resolution, cells per side, gutter, padding): face counts 72, 32, 18
ATLAS_CASES = ((96, 6, 1, 4), (64, 4, 2, 16), (48, 3, 1, 2))


def atlas_mask(resolution, n, gutter):
    from garmentdreamer_amd import texture_bake
    vt, ft = texture_bake.grid_atlas(2 * n * n, resolution, gutter)
    return chart_coverage(vt, ft, resolution, resolution)
