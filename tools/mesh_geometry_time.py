"""Time the deformer's geometry terms (garmentdreamer_amd/mesh_geometry.py, include/gd_mesh_geometry.h) and one
``Deformer.step`` on one GPU, next to the same terms written as the reference's torch composition
(deformer/core/mesh.py compute_normals, losses/laplacian.py with the sparse uniform Laplacian, losses/normal_consistency.py)
on the same GPU, on the 49 920-triangle open tube ``tube(192, 130)``; the step renders one view at 512 x 512.

    python tools/mesh_geometry_time.py [--res 512] [--iters 50]

Prints one JSON line: ``{name: {"hip_us": ..., "torch_us": ...}}``.  The method is tools/mesh_render_time.py's: medians of
HIP-event intervals on the current stream around the Python calls (autograd and allocations included), 5 warm-up runs.  A
backward is timed on a retained graph.  ``deformer_step``'s torch column is the same step (same render, same FlatAdam) with
the normals and the two geometry losses replaced by the torch composition."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from garmentdreamer_amd import mesh_geometry as mg  # noqa: E402
from garmentdreamer_amd import mesh_render as mr  # noqa: E402
from garmentdreamer_amd.deformer import CHANNELS, Deformer  # noqa: E402
from mesh_render_time import look_at, median_us, tube  # noqa: E402


def torch_normals(vertices, indices):
    """The op sequence of Mesh.compute_normals: three gathers, cross, normalize, three index_add, normalize."""
    p0, p1, p2 = (vertices[indices][:, k] for k in range(3))
    fn = torch.nn.functional.normalize(torch.linalg.cross(p1 - p0, p2 - p0), dim=-1)
    acc = torch.zeros_like(vertices)
    for k in range(3):
        acc = acc.index_add(0, indices[:, k], fn)
    return fn, torch.nn.functional.normalize(acc, dim=-1)


def torch_laplacian_matrix(edges, V, dev):
    """The uniform Laplacian as a sparse matrix: L[i, j] = 1 / deg(i) on edges, -1 on the diagonal."""
    e0, e1 = edges.unbind(1)
    idx = torch.cat([torch.stack([e0, e1], dim=1), torch.stack([e1, e0], dim=1)], dim=0).t()
    deg = torch.zeros(V, device=dev).index_add(0, idx[0], torch.ones(idx.shape[1], device=dev))
    val = 1.0 / deg[idx[0]]
    diag = torch.arange(V, device=dev)
    idx = torch.cat([idx, torch.stack([diag, diag], dim=0)], dim=1)
    val = torch.cat([val, -torch.ones(V, device=dev)])
    return torch.sparse_coo_tensor(idx, val, (V, V)).coalesce()


def torch_laplacian_loss(L, vertices):
    return (L.mm(vertices).norm(dim=1) ** 2).mean()


def torch_consistency_loss(face_normals, connected_faces):
    f, g = connected_faces.unbind(1)
    cos = torch.cosine_similarity(face_normals[f], face_normals[g], dim=1)
    return ((1 - cos) ** 2).mean()


def pair(hip, ref, iters):
    out = {"hip_us": median_us(hip, iters)}
    try:
        out["torch_us"] = median_us(ref, iters)
    except Exception as e:   # the composition, not this package: report it and go on
        out["torch_us"] = None
        out["torch_error"] = repr(e)[:200]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--nu", type=int, default=192)
    ap.add_argument("--nv", type=int, default=130)
    args = ap.parse_args()
    dev = "cuda:0"
    v_np, tri_np, _ = tube(args.nu, args.nv)
    rng = np.random.RandomState(0)
    v = torch.from_numpy(v_np + rng.normal(0, 1e-3, v_np.shape).astype(np.float32)).to(dev)
    tri = torch.from_numpy(tri_np).to(dev)
    idx64 = tri.long()
    V = v.shape[0]
    geo = mg.build_geometry(tri, num_vertices=V, device=dev)
    L = torch_laplacian_matrix(geo.edges, V, dev)
    w_vn, w_fn = torch.rand(V, 3, device=dev), torch.rand(tri.shape[0], 3, device=dev)

    def graphs(normals_fn, lap_fn, nc_fn):
        x = v.clone().requires_grad_(True)
        fn, vn = normals_fn(x)
        fn_leaf = fn.detach().clone().requires_grad_(True)
        return x, (fn * w_fn).sum() + (vn * w_vn).sum(), lap_fn(x), fn_leaf, nc_fn(fn_leaf)

    hip = graphs(lambda x: mg.normals(x, geo), lambda x: mg.laplacian_loss(x, geo),
                 lambda f: mg.normal_consistency_loss(f, geo))
    ref = graphs(lambda x: torch_normals(x, idx64), lambda x: torch_laplacian_loss(L, x),
                 lambda f: torch_consistency_loss(f, geo.connected_faces))
    fn_d = hip[3].detach()

    def backward(leaf, loss):
        def run():
            leaf.grad = None
            loss.backward(retain_graph=True)
        return run

    res = {"triangles": int(tri.shape[0]), "vertices": V, "edges": int(geo.edges.shape[0]), "pairs": geo.num_pairs,
           "resolution": args.res}
    res["normals_forward"] = pair(lambda: mg.normals(v, geo), lambda: torch_normals(v, idx64), args.iters)
    res["normals_backward"] = pair(backward(hip[0], hip[1]), backward(ref[0], ref[1]), args.iters)
    res["laplacian_forward"] = pair(lambda: mg.laplacian_loss(v, geo), lambda: torch_laplacian_loss(L, v), args.iters)
    res["laplacian_backward"] = pair(backward(hip[0], hip[2]), backward(ref[0], ref[2]), args.iters)
    res["consistency_forward"] = pair(lambda: mg.normal_consistency_loss(fn_d, geo),
                                      lambda: torch_consistency_loss(fn_d, geo.connected_faces), args.iters)
    res["consistency_backward"] = pair(backward(hip[3], hip[4]), backward(ref[3], ref[4]), args.iters)

    # one deformer iteration, one view
    pose, proj = look_at((1.5, 0.4, 1.45)), mr.perspective(0.75)
    mvp = torch.from_numpy((proj @ np.linalg.inv(pose)).astype(np.float32)).to(dev)
    h = w = args.res
    deformer = Deformer(v, tri, [mvp], [torch.zeros(h, w, 1, device=dev)], (h, w))
    with torch.no_grad():
        moved = v + torch.tensor([0.05, 0.0, 0.0], device=dev)
        deformer.target_masks = [deformer.renderer.render([mvp], moved, tri, None, (h, w), ["mask"],
                                                          topology=geo.topology)[0]["mask"]]
    weights = deformer.weights

    def torch_step():
        deformer.offsets.grad = None
        vertices = deformer.initial + deformer.offsets
        fn, vn = torch_normals(vertices, idx64)
        gbuffers = deformer.renderer.render([mvp], vertices, tri, vn, [(h, w)], CHANNELS, with_antialiasing=True,
                                            topology=geo.topology)
        loss = (weights["mask"] * mg.mask_loss(deformer.target_masks, gbuffers)
                + weights["normal_consistency"] * torch_consistency_loss(fn, geo.connected_faces)
                + weights["laplacian"] * torch_laplacian_loss(L, vertices))
        loss.backward()
        deformer.optimizer.step()

    res["deformer_step"] = pair(lambda: deformer.step([0]), torch_step, args.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
