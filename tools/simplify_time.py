"""Time one ``Deformer.final_mesh()`` (garmentdreamer_amd/mesh_simplify.py, include/gd_mesh_simplify.h) on one GPU: the
jittered ``tube(256, 128)`` of tools/remesh_time.py after one ``Deformer.remesh()`` (about 253 000 faces), rotated, decimated
to 40 000 faces and Taubin-smoothed, as the deformer stage's last line runs it.

    python tools/simplify_time.py [--nu 256] [--nv 128] [--target 40000] [--runs 3]

Prints one JSON line: the wall-clock seconds of each run (a decimation reads counts back, so it ends synchronised; one
untimed warm-up run first), the faces before and after, the rounds, the collapses selected per round, the host reads per
round (counted, not assumed: every ``Tensor.tolist`` of a run divided by its rounds) and ``reached``.  A record, not a
criterion: the operation is new, so there is no earlier figure, and pymeshlab is not available to compare with."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from garmentdreamer_amd import mesh_simplify as ms  # noqa: E402
from garmentdreamer_amd.deformer import Deformer  # noqa: E402
from remesh_time import jittered  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=256)
    ap.add_argument("--nv", type=int, default=128)
    ap.add_argument("--target", type=int, default=40000)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda:0"
    v, tri = (torch.from_numpy(a).to(dev) for a in jittered(args.nu, args.nv))
    res = (64, 64)
    d = Deformer(v, tri, [torch.eye(4, device=dev)], [torch.zeros(res + (1,), device=dev)], res)
    d.begin_second_stage([torch.full(res + (3,), 0.5, device=dev)], [torch.eye(3, device=dev)], [torch.zeros(3, device=dev)])
    d.remesh()
    out = {"faces": int(d.geometry.tri.shape[0]), "vertices": int(d.initial.shape[0]), "target": args.target, "seconds": []}
    reads, real = [0], torch.Tensor.tolist

    def counted(self):
        reads[0] += 1
        return real(self)

    for run in range(args.runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fv, ft = d.final_mesh(target_faces=args.target)
        torch.cuda.synchronize()
        if run:
            out["seconds"].append(round(time.perf_counter() - t0, 3))
    torch.Tensor.tolist = counted                                       # one more run, untimed, for the counts and the info
    try:
        _, _, info = ms.post_process_mesh((d.initial + d.offsets).detach(), d.geometry.tri, args.target)
    finally:
        torch.Tensor.tolist = real
    rounds = len(info["selected"])
    out.update(faces_after=int(ft.shape[0]), vertices_after=int(fv.shape[0]), reached=info["reached"], rounds=rounds,
               host_reads=reads[0], host_reads_per_round=round(reads[0] / max(rounds, 1), 2), selected=info["selected"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
