"""Time the second stage's G-buffer losses (garmentdreamer_amd/mesh_losses.py, include/gd_mesh_losses.h) for one view and
one ``Deformer.step_second`` on one GPU, next to the same terms written as the reference's torch composition
(deformer/losses/normal.py, losses/mask.py: elementwise ops ending in a boolean-mask gather) on the same GPU, on G-buffers
rendered from the 49 920-triangle open tube ``tube(192, 130)``; the losses at 1024 x 1024, the step at 512 x 512.

    python tools/mesh_losses_time.py [--loss-res 1024] [--res 512] [--iters 50]

Prints one JSON line: ``{name: {"hip_us": ..., "torch_us": ...}}``.  The method is tools/mesh_render_time.py's: medians of
HIP-event intervals on the current stream around the Python calls (autograd and allocations included), 5 warm-up runs.  A
backward is timed on a retained graph.  ``step_second``'s torch column is the same step (same renders, same update) with
the two G-buffer losses replaced by the torch composition; ``torch_step_trips_sync_debug`` says whether that step raises
under ``torch.cuda.set_sync_debug_mode("error")``, ``hip_step_trips_sync_debug`` the same of ``step_second``."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from garmentdreamer_amd import mesh_geometry as mg  # noqa: E402
from garmentdreamer_amd import mesh_losses as ml  # noqa: E402
from garmentdreamer_amd import mesh_render as mr  # noqa: E402
from garmentdreamer_amd.deformer import CHANNELS, Deformer  # noqa: E402
from mesh_geometry_time import pair  # noqa: E402
from mesh_render_time import look_at, tube  # noqa: E402

F = torch.nn.functional


def _flip(dev):
    return torch.diag(torch.tensor([1.0, -1.0, -1.0], device=dev))


def _direction(view, position):
    return F.normalize(view.center - position, dim=-1) @ view.R.T @ _flip(position.device).T * -1


def torch_enhanced(view, g, epsilon=-0.1):
    normal = g["normal"] @ view.R.T @ _flip(view.R.device).T
    target = view.normal * 2 - 1
    errors = 1 - F.cosine_similarity(target, normal, dim=-1)
    with torch.no_grad():
        d = _direction(view, g["position"])
        ct = F.cosine_similarity(d, target, dim=-1, eps=1e-6)
        ct[ct > epsilon] = 0
        cv = F.cosine_similarity(d, normal, dim=-1, eps=1e-6)
    weight = torch.exp(ct.abs())
    errors = errors * weight / weight.sum()
    keep = (view.mask.squeeze() > 0) & (g["mask"].squeeze() > 0) & (cv <= 0) & (ct <= epsilon)
    return errors[keep].sum()


def torch_plain(view, g):
    keep = ((view.mask > 0) & (g["mask"] > 0)).squeeze()
    normal = 0.5 * (g["normal"] @ view.R.T @ _flip(view.R.device).T + 1)[keep]
    return F.l1_loss(normal, view.normal[keep])


def torch_hole(view, g, g_rf):
    flip = _flip(view.R.device).T
    cos = F.cosine_similarity(_direction(view, g["position"]), g["normal"] @ view.R.T @ flip, dim=-1, eps=1e-6)
    cos_rf = F.cosine_similarity(_direction(view, g_rf["position"]), g_rf["normal"] @ view.R.T @ flip, dim=-1, eps=1e-6)
    for c in (cos, cos_rf):
        c.data.masked_fill_(c < 0, -1)
        c.data.masked_fill_(c >= 0, 1)
    keep = (g["mask"].squeeze() > 0) & (g_rf["mask"].squeeze() > 0)
    return F.mse_loss(cos[keep], cos_rf[keep])


def trips_sync_debug(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        fn()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss-res", type=int, default=1024)
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
    geo = mg.build_geometry(tri, num_vertices=v.shape[0], device=dev)
    pose, proj = look_at((1.5, 0.4, 1.45)), mr.perspective(0.75)
    mvp = torch.from_numpy((proj @ np.linalg.inv(pose)).astype(np.float32)).to(dev)
    flip = np.diag([1.0, -1.0, -1.0])
    R = torch.from_numpy((flip @ pose[:3, :3].T.astype(np.float64)).astype(np.float32)).to(dev)
    center = torch.from_numpy(pose[:3, 3].astype(np.float32)).to(dev)
    moved = v + torch.tensor([0.05, 0.0, 0.0], device=dev)

    def target(res):
        deformer = Deformer(v, tri, [mvp], [torch.zeros(res, res, 1, device=dev)], (res, res))
        with torch.no_grad():
            g = deformer.renderer.render([mvp], moved, tri, mg.normals(moved, geo)[1], (res, res), ["mask", "normal"],
                                         topology=geo.topology)[0]
        deformer.target_masks = [g["mask"]]
        return deformer, (0.5 * (g["normal"] @ R.T @ _flip(dev).T + 1)).contiguous()

    res = {"triangles": int(tri.shape[0]), "vertices": int(v.shape[0]), "loss_resolution": args.loss_res,
           "step_resolution": args.res}

    # the three losses of one view
    n = args.loss_res
    deformer, normal_map = target(n)
    view = ml.View(normal_map, deformer.target_masks[0], R, center)
    with torch.no_grad():
        shifted = v + torch.from_numpy(rng.normal(0, 5e-3, v_np.shape).astype(np.float32)).to(dev)
        g0 = deformer.renderer.render([mvp], v, tri, mg.normals(v, geo)[1], (n, n), CHANNELS, topology=geo.topology)[0]
        g_rf = deformer.renderer.render([mvp], shifted, tri, mg.normals(shifted, geo)[1], (n, n), CHANNELS,
                                        topology=geo.topology)[0]

    def leaves():
        return {"normal": g0["normal"].clone().requires_grad_(True), "position": g0["position"].clone().requires_grad_(True),
                "mask": g0["mask"]}

    def backward(g, loss):
        def run():
            g["normal"].grad = g["position"].grad = None
            loss.backward(retain_graph=True)
        return run

    terms = {"enhanced": (lambda g: ml.normal_map_loss_enhanced([view], [g]), lambda g: torch_enhanced(view, g)),
             "plain": (lambda g: ml.normal_map_loss([view], [g]), lambda g: torch_plain(view, g)),
             "hole": (lambda g: ml.hole_mask_loss([view], [g], [g_rf]), lambda g: torch_hole(view, g, g_rf)),
             "all_three": (lambda g: sum(ml.second_stage_losses([view], [g], [g_rf])[k]
                                         for k in ("normal_enhanced", "normal_plain", "hole_mask")),
                           lambda g: torch_enhanced(view, g) + torch_plain(view, g) + torch_hole(view, g, g_rf))}
    for name, (hip, ref) in terms.items():
        g_hip, g_ref = leaves(), leaves()
        res[name + "_forward"] = pair(lambda: hip(g_hip), lambda: ref(g_ref), args.iters)
        res[name + "_backward"] = pair(backward(g_hip, hip(g_hip)), backward(g_ref, ref(g_ref)), args.iters)
        res[name + "_values"] = [float(hip(g_hip).detach()), float(ref(g_ref).detach())]

    # one second-stage iteration, one view
    h = args.res
    deformer, normal_map = target(h)
    for _ in range(3):
        deformer.step([0])
    deformer.begin_second_stage([normal_map], [R], [center])
    view = deformer.views[0]
    weights = deformer.second_weights

    def torch_step():
        deformer.offsets.grad = None
        vertices = deformer.initial + deformer.offsets
        fn, vn = mg.normals(vertices, geo)
        gb = deformer.renderer.render([mvp], vertices, tri, vn, [(h, h)], CHANNELS, with_antialiasing=True,
                                      topology=geo.topology)
        with torch.no_grad():
            rf = deformer.renderer.render([mvp], deformer.rf_vertices, tri, deformer.rf_normals, [(h, h)], CHANNELS,
                                          with_antialiasing=True, topology=geo.topology)
        loss = (weights["mask"] * mg.mask_loss(deformer.target_masks, gb)
                + weights["normal_consistency"] * mg.normal_consistency_loss(fn, geo)
                + weights["laplacian"] * mg.laplacian_loss(vertices, geo)
                + weights["normal"] * torch_enhanced(view, gb[0]) + weights["hole_mask"] * torch_hole(view, gb[0], rf[0]))
        loss.backward()
        deformer._step_visible([mvp], vertices, [(h, h)])

    res["step_second"] = pair(lambda: deformer.step_second([0]), torch_step, args.iters)
    res["hip_step_trips_sync_debug"] = trips_sync_debug(lambda: deformer.step_second([0]))
    res["torch_step_trips_sync_debug"] = trips_sync_debug(torch_step)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
