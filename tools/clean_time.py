"""Time one ``mesh_clean.clean_mesh`` (garmentdreamer_amd/mesh_clean.py, include/gd_mesh_clean.h) on one GPU: the jittered
tube of tools/remesh_time.py at about 200 000 faces plus injected junk -- duplicated faces, 50 fragments, 100 pinched
vertices, a 3-page book strip, near-duplicate vertices -- with the reference's ``min_faces=32``, ``min_diameter_pct=10``.

    python tools/clean_time.py [--nu 400] [--nv 250] [--merge-pct 0.05] [--runs 3]

Prints one JSON line: the wall-clock milliseconds of each whole run (one untimed warm-up first), then from one more run
with a device synchronisation around every step the milliseconds per step, the milliseconds inside ``torch.sort`` and their
share, the host reads (every ``Tensor.tolist`` and ``Tensor.cpu``, counted), the report, and as the yardstick the
milliseconds of a device copy of the mesh's bytes.  ``--merge-pct`` defaults to a radius below the tube's edge length, which
welds the injected near-duplicates only; at kiui's default of 1 percent the radius is about three edges of this tube and
the weld itself takes hundreds of rounds.  A record, not a criterion: the operation is new, so there is no earlier figure,
and pymeshlab is not available to compare with."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from garmentdreamer_amd import mesh_clean as mc  # noqa: E402
from remesh_time import jittered  # noqa: E402

STEPS = ("_check", "_merge", "_relabel", "_edge_table", "_duplicates", "_face_parents", "_component_filter", "_edge_rounds",
         "_corner_parents", "_emit")


def with_junk(v, tri, nu, seed=0):
    rng = np.random.RandomState(seed)
    v, tri = v.astype(np.float32), tri.astype(np.int64)
    V0, F0 = v.shape[0], tri.shape[0]
    size = float(np.linalg.norm(v.max(0) - v.min(0)))
    parts_v, parts_t = [v], [tri]
    dup = tri[rng.choice(F0, 1000, replace=False)]
    parts_t.append(np.concatenate((dup[:500][:, [1, 2, 0]], dup[500:][:, [2, 1, 0]])))        # duplicated faces
    at = V0
    for k in range(50):                                                  # fragments: fans of 6 faces off the surface
        c = v[rng.randint(V0)] * 1.3
        ang = 2 * np.pi * np.arange(6) / 6
        rim = c + 0.01 * size * np.stack((np.cos(ang), np.sin(ang), 0 * ang), axis=1)
        parts_v.append(np.concatenate((c[None], rim)).astype(np.float32))
        parts_t.append(np.array([(at, at + 1 + i, at + 1 + (i + 1) % 6) for i in range(6)]))
        at += 7
    row = nu * 40                                                        # a 3-page book strip along 60 edges of one ring
    for i in range(60):
        a, b = row + i, row + i + 1
        parts_v.append((0.5 * (v[a] + v[b]) * np.float32((1.05, 1.05, 1.0)))[None])
        parts_t.append(np.array([(a, b, at)]))
        at += 1
    near = rng.choice(F0, 200, replace=False)                            # near-duplicate vertices, each used by one face
    for f in near:
        parts_v.append((v[tri[f, 0]] + 1e-5 * size * rng.uniform(-1, 1, 3)).astype(np.float32)[None])
        parts_t.append(np.array([(at, tri[f, 1], tri[f, 2])]))
        at += 1
    v, tri = np.concatenate(parts_v).astype(np.float32), np.concatenate(parts_t)
    pairs = rng.choice(np.arange(nu, V0 - nu), (100, 2), replace=False)  # pinched vertices: two interior vertices named as one
    for x, y in pairs:
        tri[tri == y] = x
    return v, tri


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nu", type=int, default=400)
    ap.add_argument("--nv", type=int, default=250)
    ap.add_argument("--merge-pct", type=float, default=0.05)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda:0"
    hv, ht = with_junk(*jittered(args.nu, args.nv), args.nu)
    v, tri = torch.from_numpy(hv).to(dev), torch.from_numpy(ht.astype(np.int32)).to(dev)
    kw = dict(merge_pct=args.merge_pct, min_faces=32, min_diameter_pct=10.0)
    out = {"faces": int(tri.shape[0]), "vertices": int(v.shape[0]), "merge_pct": args.merge_pct, "ms": []}
    for run in range(args.runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = mc.clean_mesh(v, tri, **kw)
        torch.cuda.synchronize()
        if run:
            out["ms"].append(round(1e3 * (time.perf_counter() - t0), 2))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        v.clone(), tri.clone()
    torch.cuda.synchronize()
    out["copy_ms"] = round(1e2 * (time.perf_counter() - t0), 4)
    # one more run with a synchronisation around every step
    spent, sort_ms, reads = {s: 0.0 for s in STEPS}, [0.0], [0]
    real = {s: getattr(mc, s) for s in STEPS}
    real_sort, real_tolist, real_cpu = torch.sort, torch.Tensor.tolist, torch.Tensor.cpu

    def timed(name, fn, into):
        def run(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            torch.cuda.synchronize()
            into(name, 1e3 * (time.perf_counter() - t0))
            return r
        return run

    def counted(fn):
        def run(self, *a, **k):
            reads[0] += 1
            return fn(self, *a, **k)
        return run

    try:
        for s in STEPS:
            setattr(mc, s, timed(s, real[s], lambda n, ms: spent.__setitem__(n, spent[n] + ms)))
        torch.sort = timed("sort", real_sort, lambda n, ms: sort_ms.__setitem__(0, sort_ms[0] + ms))
        torch.Tensor.tolist, torch.Tensor.cpu = counted(real_tolist), counted(real_cpu)
        res = mc.clean_mesh(v, tri, **kw)
    finally:
        for s in STEPS:
            setattr(mc, s, real[s])
        torch.sort, torch.Tensor.tolist, torch.Tensor.cpu = real_sort, real_tolist, real_cpu
    total = sum(spent.values())
    out.update(step_ms={s.strip("_"): round(ms, 3) for s, ms in spent.items()}, steps_total_ms=round(total, 2),
               sort_ms=round(sort_ms[0], 3), sort_share=round(sort_ms[0] / total, 3), host_reads=reads[0],
               faces_after=int(res.indices.shape[0]), vertices_after=int(res.vertices.shape[0]), report=res.report)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
