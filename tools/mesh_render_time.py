"""Time the mesh render path (garmentdreamer_amd/mesh_render.py, mesh_deform.py) on one GPU: each entry point of
include/gd_mesh.h and include/gd_mesh_deform.h on its own, one ``MeshRenderer.render`` and its backward, one
``GBufferRenderer.render`` and its backward to the vertices, at 512 x 512 on a generated open tube of about 50 000 triangles.

    python tools/mesh_render_time.py [--res 512] [--iters 50]

Prints one JSON line.  Times are medians of HIP-event intervals on the current stream, in microseconds; an entry point
is one to three kernels (rasterize: memsets + small + large + resolve; interpolate backward: corner_grad + vertex_sum;
the two position gradients: one wave-per-triangle kernel + vertex_sum)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from garmentdreamer_amd import mesh_deform as md  # noqa: E402
from garmentdreamer_amd import mesh_render as mr  # noqa: E402


def tube(nu, nv, r=0.3, h=1.0):
    ang = 2.0 * np.pi * np.arange(nu) / nu
    v = np.array([[r * np.cos(a), r * np.sin(a), h * j / nv] for j in range(nv + 1) for a in ang], dtype=np.float32)
    q = np.array([[j * nu + i, j * nu + (i + 1) % nu, (j + 1) * nu + (i + 1) % nu, (j + 1) * nu + i]
                  for j in range(nv) for i in range(nu)], dtype=np.int32)
    vn = np.array([[np.cos(a), np.sin(a), 0.0] for _ in range(nv + 1) for a in ang], dtype=np.float32)
    return v, np.concatenate((q[:, [0, 1, 2]], q[:, [0, 2, 3]])), vn


def look_at(campos, target=(0.0, 0.0, 0.5), up=(0.0, 0.0, 1.0)):
    campos, target, up = (np.asarray(a, dtype=np.float64) for a in (campos, target, up))
    z = campos - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, np.cross(z, x), z, campos
    return pose.astype(np.float32)


def median_us(fn, iters):
    for _ in range(5):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return round(float(np.median(times)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--nu", type=int, default=160)
    ap.add_argument("--nv", type=int, default=156)
    args = ap.parse_args()
    dev = "cuda:0"
    v, tri, vn = (torch.from_numpy(a).to(dev) for a in tube(args.nu, args.nv))
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(3, 32), torch.nn.ReLU(), torch.nn.Linear(32, 3), torch.nn.Sigmoid()).to(dev)
    renderer = mr.MeshRenderer(v, tri, vn, net)
    pose, proj = look_at((1.5, 0.4, 1.45)), mr.perspective(0.75)
    h = w = args.res
    _, pos = renderer.clip_positions(pose, proj)
    topo = renderer.topology
    rast = mr.rasterize(pos, tri, (h, w))
    wts = mr.antialias_weights(rast, pos, tri, topo)
    img = torch.rand(h, w, 3, device=dev)
    attr = v.clone().requires_grad_(True)
    out = mr.interpolate(attr, rast, tri, pos=pos, topology=topo)
    g = torch.rand_like(out)
    img_g = img.clone().requires_grad_(True)
    aa = mr.antialias(img_g, rast, pos, tri, weights=wts)

    # moving geometry: the gradient to rast alone, the rasterize backward alone, the antialias gradient to pos alone
    rast_leaf = rast.clone().requires_grad_(True)
    out_r = md.interpolate(v, rast_leaf, tri, pos, topo)
    pos_leaf = pos.clone().requires_grad_(True)
    rast_m = md.rasterize(pos_leaf, tri, (h, w), topo)
    g_rast = torch.rand_like(rast_m)
    pos_aa = pos.clone().requires_grad_(True)
    aa_m = md.antialias(img, rast, pos_aa, tri, topo, weights=wts)
    mask = torch.clamp(rast[..., -1:], 0, 1).contiguous()
    aa_mask = md.antialias(mask, rast, pos_aa, tri, topo, weights=wts)
    g_mask = torch.rand_like(aa_mask)
    gbuf = md.GBufferRenderer()
    mvp = torch.from_numpy(proj @ np.linalg.inv(pose)).to(dev)
    verts = v.clone().requires_grad_(True)
    channels = ["mask", "position", "normal"]

    def gbuffer_backward():
        verts.grad = None
        out = gbuf.render([mvp], verts, tri, vn, (h, w), channels, topology=topo)[0]
        (((out["mask"] - 0.5) ** 2).mean() + ((out["position"] - img) ** 2).mean()
         + ((out["normal"] - img) ** 2).mean()).backward()

    def render_backward():
        net.zero_grad(set_to_none=True)
        ((renderer.render(pose, proj, h, w)["image"] - img) ** 2).mean().backward()

    res = {
        "triangles": int(tri.shape[0]), "resolution": h, "covered_fraction": round(float((rast[..., 3] > 0).float().mean()), 3),
        "rasterize_us": median_us(lambda: mr.rasterize(pos, tri, (h, w)), args.iters),
        "antialias_weights_us": median_us(lambda: mr.antialias_weights(rast, pos, tri, topo), args.iters),
        "interpolate_forward_c3_us": median_us(lambda: mr.interpolate(v, rast, tri), args.iters),
        "interpolate_backward_c3_us": median_us(lambda: out.backward(g, retain_graph=True), args.iters),
        "antialias_apply_c3_us": median_us(lambda: mr.antialias(img, rast, pos, tri, weights=wts), args.iters),
        "antialias_adjoint_c3_us": median_us(lambda: aa.backward(g, retain_graph=True), args.iters),
        "interpolate_backward_rast_c3_us": median_us(lambda: out_r.backward(g, retain_graph=True), args.iters),
        "rasterize_backward_us": median_us(lambda: rast_m.backward(g_rast, retain_graph=True), args.iters),
        "antialias_backward_pos_c3_us": median_us(lambda: aa_m.backward(g, retain_graph=True), args.iters),
        "antialias_backward_pos_c1_us": median_us(lambda: aa_mask.backward(g_mask, retain_graph=True), args.iters),
        "visible_vertices_us": median_us(lambda: md.visible_vertices(rast, tri, v.shape[0]), args.iters),
        "gbuffer_render_us": median_us(lambda: gbuf.render([mvp], verts, tri, vn, (h, w), channels, topology=topo),
                                       args.iters),
        "gbuffer_render_and_backward_us": median_us(gbuffer_backward, args.iters),
        "render_us": median_us(lambda: renderer.render(pose, proj, h, w), args.iters),
        "render_and_backward_us": median_us(render_backward, args.iters),
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
