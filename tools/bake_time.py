"""Time the texture bake (garmentdreamer_amd/texture_bake.py, include/gd_bake.h) on one GPU: the padding kernel, the
resolve and the whole ``bake_texture`` at 2048 x 2048 with ``padding`` 16, on a ``grid_atlas`` of the 49 920-triangle
``tube(192, 130)`` and the production texture field; next to them the scipy / scikit-learn formulation of the padding
(what kiui's ``uv_padding(..., backend='knn')`` is understood to do) on the host, on the same mask.

    python tools/bake_time.py [--res 2048] [--padding 16] [--iters 50] [--no-host]

Prints one JSON line.  The method is tools/mesh_render_time.py's: medians of HIP-event intervals on the current stream
around the Python calls (allocations included), 5 warm-up runs.  The host formulation is timed ONCE with the wall clock,
the copy of the image and the mask to the host not included."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from garmentdreamer_amd import texture_bake as tb  # noqa: E402
from garmentdreamer_amd import texture_field as tf  # noqa: E402
from mesh_render_time import median_us, tube  # noqa: E402


def host_padding(image, mask, padding):
    """binary dilation (4-connected, ``padding`` iterations) minus the mask is the region; one KD-tree neighbour among the
    mask's two outer layers"""
    from scipy.ndimage import binary_dilation, binary_erosion
    from sklearn.neighbors import NearestNeighbors
    region = binary_dilation(mask, iterations=padding) & ~mask
    search = mask & ~binary_erosion(mask, iterations=2)
    search_coords = np.stack(np.nonzero(search), axis=-1)
    fill_coords = np.stack(np.nonzero(region), axis=-1)
    _, found = NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(search_coords).kneighbors(fill_coords)
    out = image.copy()
    out[tuple(fill_coords.T)] = image[tuple(search_coords[found[:, 0]].T)]
    return out, int(region.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--padding", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--nu", type=int, default=192)
    ap.add_argument("--nv", type=int, default=130)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    fld = tf.TextureField(generator=torch.Generator().manual_seed(0)).to(dev)
    v, tri, _ = (torch.from_numpy(a).to(dev) for a in tube(args.nu, args.nv))
    vt, ft = tb.grid_atlas(tri.shape[0], args.res)
    baked = tb.bake_texture(fld, v, tri, vt, ft, args.res, args.padding)
    mask, src = baked["mask"], baked["src"]
    color = torch.rand(args.res, args.res, 3, device=dev)
    res = {"resolution": args.res, "padding": args.padding, "triangles": int(tri.shape[0]), "iters": args.iters,
           "covered_texels": int(mask.sum()), "filled_texels": int(((src >= 0) & ~mask).sum())}
    res["pad_index_us"] = median_us(lambda: tb.uv_padding_index(mask, args.padding), args.iters)
    for p in (4, 64):
        res[f"pad_index_p{p}_us"] = median_us(lambda: tb.uv_padding_index(mask, p), args.iters)
    res["resolve_u8_us"] = median_us(lambda: tb.resolve_u8(color, src), args.iters)
    res["bake_texture_us"] = median_us(lambda: tb.bake_texture(fld, v, tri, vt, ft, args.res, args.padding), args.iters)
    if not args.no_host:
        image, m = color.cpu().numpy(), mask.cpu().numpy()
        t0 = time.perf_counter()
        padded, region = host_padding(image, m, args.padding)
        res["host_knn_padding_s"] = round(time.perf_counter() - t0, 2)
        res["host_region_texels"] = region
        s = src.cpu().numpy()
        ours = image.reshape(-1, 3)[np.maximum(s, 0).ravel()].reshape(image.shape)
        fill = (s >= 0) & ~m
        res["host_differs_on_filled_texels"] = int((ours[fill] != padded[fill]).any(axis=1).sum())   # its ties
    print(json.dumps(res))


if __name__ == "__main__":
    main()
