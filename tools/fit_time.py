"""Time the texture fit's loss head (garmentdreamer_amd/texture_fit.py, include/gd_fit.h) and one whole fit iteration on one
GPU, next to the reference's composition in torch on the same GPU (``NeTFRenderer.render`` -> the three masks -> the
boolean gather -> ``MSELoss``, mesh_renderer.py:224-234), on the open tube of tests/mesh_scenes.py.

    python tools/fit_time.py [--res 1024 512] [--iters 20] [--nu 24] [--nv 12]

Prints one JSON line: per resolution ``head`` (``fit_loss`` forward + backward on buffers rendered once, against the tail
of the render and the gathered MSE on the same buffers) and ``iteration`` (buffers or render, loss, backward, the
optimizer's step and ``zero_grad``), each ``{"hip_us": ..., "torch_us": ...}``: medians of HIP-event intervals on the current
stream around the Python calls (autograd and allocations included), 5 warm-up runs, the two columns one after the other.
``*_trips_sync_debug`` says whether the iteration raises under ``torch.cuda.set_sync_debug_mode("error")``."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from garmentdreamer_amd import mesh_render as mr  # noqa: E402
from garmentdreamer_amd import texture_field as tf  # noqa: E402
from garmentdreamer_amd import texture_fit as fit  # noqa: E402
from mesh_geometry_time import pair  # noqa: E402
from mesh_losses_time import trips_sync_debug  # noqa: E402
from tests import mesh_scenes as scenes  # noqa: E402


def torch_tail(b, rgb, mask, bg=1.0):
    """the tail of Renderer.render on the buffers ``b`` and the fit's loss, as the reference composes them"""
    alpha = b.a_aa[..., None].clamp(0, 1)
    image = alpha * b.c_aa.clamp(0, 1) + (1 - alpha) * bg
    with torch.no_grad():
        view_direction = F.normalize(b.p_aa - b.center, dim=-1)
        cosines = F.cosine_similarity(view_direction, b.n_aa, dim=-1, eps=1e-6)
    keep = (alpha.squeeze() > 0) & (torch.flipud(mask.squeeze()) > 0) & (cosines <= 0)
    return F.mse_loss(image[keep], torch.flipud(rgb)[keep])


def torch_loss(out, rgb, mask):
    keep = (out["alpha"].squeeze() > 0) & (torch.flipud(mask.squeeze()) > 0) & (out["cosinesview"] <= 0)
    return F.mse_loss(out["image"][keep], torch.flipud(rgb)[keep])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[1024, 512])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--nu", type=int, default=24)
    ap.add_argument("--nv", type=int, default=12)
    args = ap.parse_args()
    dev = "cuda:0"
    v, tri, vn = (torch.from_numpy(a).to(dev) for a in scenes.tube(args.nu, args.nv))
    torch.manual_seed(0)
    field = tf.TextureField(generator=torch.Generator().manual_seed(1)).to(dev)
    netf = tf.NeTFRenderer(v, tri, vn, field)
    opt = field.optimizer()
    pose, proj = scenes.look_at_pose(scenes.CAMPOS), mr.perspective(scenes.FOVY)
    res = {"triangles": int(tri.shape[0]), "iters": args.iters}
    for n in args.res:
        rgb = torch.rand(n, n, 3, device=dev)
        mask = (torch.rand(n, n, 1, device=dev) > 0.2).float()
        with torch.no_grad():
            rendered = fit.fit_buffers(netf, pose, proj, n, n)

        def head(loss_fn):
            b = rendered._replace(c_aa=rendered.c_aa.clone().requires_grad_(True))

            def run():
                b.c_aa.grad = None
                loss_fn(b, rgb, mask).backward()
            return run

        def hip_iteration():
            loss = fit.fit_loss(fit.fit_buffers(netf, pose, proj, n, n), rgb, mask)
            loss.backward()
            opt.step()
            opt.zero_grad()
            return loss.detach()

        def torch_iteration():
            loss = torch_loss(netf.render(pose, proj, n, n), rgb, mask)
            loss.backward()
            opt.step()
            opt.zero_grad()
            return loss.detach()

        opt.zero_grad()
        values = [float(fit.fit_loss(rendered, rgb, mask)), float(torch_tail(rendered, rgb, mask)),
                  float(torch_loss(netf.render(pose, proj, n, n), rgb, mask).detach())]
        opt.zero_grad()
        res[str(n)] = {"head": pair(head(fit.fit_loss), head(torch_tail), args.iters),
                       "iteration": pair(hip_iteration, torch_iteration, args.iters),
                       "values_hip_tail_render": values,
                       "selected": int(fit.fit_loss(rendered, rgb, mask, outputs=True)[3].sum()),
                       "hip_trips_sync_debug": trips_sync_debug(hip_iteration),
                       "torch_trips_sync_debug": trips_sync_debug(torch_iteration)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
