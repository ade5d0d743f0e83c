"""Time one ``Deformer.remesh()`` (garmentdreamer_amd/mesh_remesh.py, include/gd_mesh_remesh.h) on one GPU: the
65 536-triangle ``tube(256, 128)`` with its inner rings jittered along the surface, h = half the mean edge length, ten
iterations, as an upsample iteration of the deformer's second stage runs it.

    python tools/remesh_time.py [--nu 256] [--nv 128] [--runs 3]

Prints one JSON line: the wall-clock seconds of each run (a remesh reads counts back, so it ends synchronised; one
untimed warm-up run first), the faces before and after and the remesher's ``info`` of the last run.  A record, not a
criterion: there is nothing to compare it with (gpytoolbox is not available here)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from garmentdreamer_amd.deformer import Deformer  # noqa: E402
from mesh_render_time import tube  # noqa: E402


def jittered(nu, nv, seed=0, amount=0.25):
    v, tri, _ = tube(nu, nv)
    rng = np.random.RandomState(seed)
    ang = np.arctan2(v[:, 1], v[:, 0]) + rng.uniform(-amount, amount, v.shape[0]) * (2.0 * np.pi / nu)
    z = v[:, 2] + rng.uniform(-amount, amount, v.shape[0]) / nv
    inner = (np.arange(v.shape[0]) >= nu) & (np.arange(v.shape[0]) < nv * nu)          # the two rims stay
    r = np.hypot(v[:, 0], v[:, 1])
    moved = np.stack((r * np.cos(ang), r * np.sin(ang), z), axis=1).astype(np.float32)
    return np.where(inner[:, None], moved, v), tri


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=256)
    ap.add_argument("--nv", type=int, default=128)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda:0"
    v, tri = (torch.from_numpy(a).to(dev) for a in jittered(args.nu, args.nv))
    res = (64, 64)
    mvp = torch.eye(4, device=dev)
    blank = torch.zeros(res + (1,), device=dev)
    out = {"faces": int(tri.shape[0]), "vertices": int(v.shape[0]), "seconds": []}
    for run in range(args.runs + 1):
        d = Deformer(v, tri, [mvp], [blank], res)
        d.begin_second_stage([torch.full(res + (3,), 0.5, device=dev)], [torch.eye(3, device=dev)], [torch.zeros(3, device=dev)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = d.remesh()
        torch.cuda.synchronize()
        if run:
            out["seconds"].append(round(time.perf_counter() - t0, 3))
        out.update(faces_after=int(d.geometry.tri.shape[0]), vertices_after=int(d.initial.shape[0]), info=info)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
