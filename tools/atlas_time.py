"""Time the phases of one ``texture_atlas.chart_atlas`` (garmentdreamer_amd/texture_atlas.py, include/gd_atlas.h) on one
GPU: a pleated tube of 40 000 faces (the size ``Deformer.final_mesh`` decimates to), generated here, unwrapped at 2048 x 2048
with a gutter of 2.

    python tools/atlas_time.py [--nu 200] [--nv 100] [--res 2048] [--gutter 2] [--runs 3]

Prints one JSON line: the milliseconds of each phase of the first round (connectivity, classes, components with their
sweep count, bounds, the host packer, corners and welding, the rasterizer, lost faces; each between two synchronisations,
best of ``runs``), the wall-clock milliseconds of the whole call (it ends on a host read), and what the atlas is: charts,
rounds, lost faces per round, seam edges, vt rows, coverage, next to ``grid_atlas``'s coverage for the same face count.  A
record, not a criterion: the operation is new, so there is no earlier figure, and xatlas is not available to compare
with."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from garmentdreamer_amd import texture_atlas as ta  # noqa: E402
from garmentdreamer_amd import texture_bake as tb  # noqa: E402
from garmentdreamer_amd.mesh_connectivity import build_connectivity  # noqa: E402


def pleated_tube(nu, nv, r=0.3, h=1.0, depth=0.03, pleats=5):
    """an open tube around z whose radius waves with the angle and the height: 2 nu nv faces"""
    ang = 2.0 * np.pi * np.arange(nu) / nu
    z = h * np.arange(nv + 1) / nv
    rad = r + depth * np.sin(pleats * ang)[None, :] * np.cos(4.0 * np.pi * z)[:, None]
    v = np.stack((rad * np.cos(ang)[None, :], rad * np.sin(ang)[None, :], np.broadcast_to(z[:, None], rad.shape)), axis=2)
    j, i = np.meshgrid(np.arange(nv), np.arange(nu), indexing="ij")
    a, b, c, d = j * nu + i, j * nu + (i + 1) % nu, (j + 1) * nu + (i + 1) % nu, (j + 1) * nu + i
    tri = np.concatenate((np.stack((a, b, c), axis=2).reshape(-1, 3), np.stack((a, c, d), axis=2).reshape(-1, 3)))
    return v.reshape(-1, 3).astype(np.float32), tri.astype(np.int32)


def timed(fn, runs):
    """(best milliseconds, the last result)"""
    best = None
    for _ in range(runs + 1):                                           # the first is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return round(best, 3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=200)
    ap.add_argument("--nv", type=int, default=100)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--gutter", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda:0"
    v, t = (torch.from_numpy(a).to(dev) for a in pleated_tube(args.nu, args.nv))
    F, res, g = t.shape[0], args.res, args.gutter
    ms = {}
    ms["connectivity"], conn = timed(lambda: build_connectivity(t, v.shape[0]), args.runs)
    ms["classes"], cls = timed(lambda: ta.face_classes(v, t), args.runs)
    ms["components"], (labels, sweeps) = timed(lambda: ta.chart_labels(conn, cls, return_sweeps=True), args.runs)
    ms["bounds"], (C, face_chart, bounds, count) = timed(lambda: ta.chart_bounds(v, t, cls, labels), args.runs)
    host = bounds.cpu().numpy()
    ms["pack_host"], (scale, offsets, sizes) = timed(lambda: ta.pack_charts(host, res, g), args.runs)
    ms["corners_weld"], (corner_xy, vt, ft) = timed(
        lambda: ta._emit(v, t, cls, face_chart, bounds, C, res, g, scale, offsets), args.runs)
    ms["rasterize"], rast = timed(lambda: ta._rasterize_atlas(vt, ft, res), args.runs)
    lost = torch.empty(F, dtype=torch.int32, device=dev)
    layer, single = torch.zeros_like(lost), torch.zeros_like(lost)
    # freeze = 1 and a scratch copy: the timed call must not move the layers
    ms["lost_faces"], _ = timed(lambda: ta.launch("gd_atlas_lost_faces", dev, F, res, res, corner_xy, rast, 1, lost,
                                                  layer.clone(), single.clone()), args.runs)
    ms["chart_atlas"], (vt, ft, info) = timed(lambda: ta.chart_atlas(v, t, res, g), args.runs)
    grid_vt, grid_ft = tb.grid_atlas(F, res)
    pos = torch.from_numpy(np.concatenate((grid_vt * 2 - 1, np.zeros_like(grid_vt[:, :1]), np.ones_like(grid_vt[:, :1])),
                                          axis=1).astype(np.float32)).to(dev)
    grid_cover = float((ta.rasterize(pos, torch.from_numpy(grid_ft).to(dev), (res, res))[..., 3] > 0).sum()) / (res * res)
    print(json.dumps({"faces": F, "resolution": res, "gutter": g, "ms": ms, "sweeps": sweeps, "charts": info["num_charts"],
                      "rounds": info["rounds"], "lost_per_round": info["lost_per_round"], "singletons": info["singletons"],
                      "seam_edges": info["seam_edges"], "interior_edges": int((conn.eh[:, 1] >= 0).sum()),
                      "vt_rows": int(vt.shape[0]), "scale": info["scale"], "coverage": round(info["coverage"], 4),
                      "grid_atlas_coverage": round(grid_cover, 4), "first_round_lost": int(lost.sum())}))


if __name__ == "__main__":
    main()
