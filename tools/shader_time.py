"""Time the neural shader and the shading loss (garmentdreamer_amd/neural_shader.py, mesh_losses.shading_loss,
include/gd_shader.h) on one GPU, stage by stage for one view and as one ``Deformer.step_second`` with and without the
shader, next to the same work written as the reference's torch composition on the same GPU: fp32 ``nn.Linear`` layers behind
a boolean-mask gather and a host ``randperm`` (deformer/losses/shading.py over deformer/modules/neuralshader.py), on
G-buffers rendered from the 49 920-triangle open tube ``tube(192, 130)`` at 1024 x 1024 and 512 x 512, 75 % of the valid
pixels.

    python tools/shader_time.py [--res 1024 512] [--iters 20]

Prints one JSON line: per resolution ``{name: {"hip_us": ..., "torch_us": ...}}`` plus the number of shaded points and the
achieved bf16 FLOP/s of the products (2 x 319 360 multiply-adds per point forward, twice that again backward).  The method
is tools/mesh_losses_time.py's: medians of HIP-event intervals on the current stream around the Python calls, 5 warm-up
runs; a backward is timed on a retained graph."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from garmentdreamer_amd import _native  # noqa: E402
from garmentdreamer_amd import mesh_geometry as mg  # noqa: E402
from garmentdreamer_amd import mesh_losses as ml  # noqa: E402
from garmentdreamer_amd import mesh_render as mr  # noqa: E402
from garmentdreamer_amd import neural_shader as ns  # noqa: E402
from garmentdreamer_amd._launch import launch, scratch  # noqa: E402
from garmentdreamer_amd.deformer import CHANNELS, Deformer  # noqa: E402
from mesh_geometry_time import pair  # noqa: E402
from mesh_losses_time import trips_sync_debug  # noqa: E402
from mesh_render_time import look_at, median_us, tube  # noqa: E402

F = torch.nn.functional
MACS = sum(k * o for k, o in zip(ns.IN_FEATURES, ns.OUT_FEATURES))
PERCENTAGE = 0.75


class TorchShader(torch.nn.Module):
    """The reference's network as plain fp32 torch with the weights of a ``NeuralShader``"""

    def __init__(self, shader):
        super().__init__()
        state = shader.state_dict()
        self.layers = torch.nn.ModuleList()
        for name, k, o in zip(ns.LAYER_NAMES, ns.IN_FEATURES, ns.OUT_FEATURES):
            layer = torch.nn.Linear(k, o, device=shader.device)
            layer.weight.data.copy_(state[name + ".weight"])
            layer.bias.data.copy_(state[name + ".bias"])
            self.layers.append(layer)

    def forward(self, position, normal, view_dir):
        h = torch.cat([position] + [fn(position * f) for f in (1.0, 2.0, 4.0, 8.0) for fn in (torch.sin, torch.cos)], dim=-1)
        for l, layer in enumerate(self.layers):
            if l == 5:
                h = torch.cat([h, normal, view_dir], dim=-1)
            h = layer(h)
            if l not in (4, 7):
                h = torch.relu(h)
        return torch.sigmoid(h)


def torch_valid(view, g):
    flip = torch.diag(torch.tensor([1.0, -1.0, -1.0], device=view.R.device))
    with torch.no_grad():
        normal = g["normal"] @ view.R.T @ flip.T
        d = -(F.normalize(view.center - g["position"], dim=-1) @ view.R.T @ flip.T)
        cv = F.cosine_similarity(d, normal, dim=-1, eps=1e-6)
    return (view.mask.squeeze() > 0) & (g["mask"].squeeze() > 0) & (cv <= 0)


def torch_gather(view, g, percentage):
    """(position, normal, view_dir, target) of the sampled valid pixels: a boolean gather and a host randperm"""
    mask = torch_valid(view, g)
    position, normal, target = g["position"][mask], g["normal"][mask], view.rgb[mask]
    if percentage != 1:
        idx = torch.randperm(position.shape[0])[:int(position.shape[0] * percentage)]
        position, normal, target = position[idx], normal[idx], target[idx]
    return position, normal, F.normalize(view.center - position, dim=-1), target


def torch_shading(view, g, shader, percentage):
    position, normal, view_dir, target = torch_gather(view, g, percentage)
    return F.l1_loss(shader(position, normal, view_dir), target)


def one_resolution(res, args, dev):
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
    deformer = Deformer(v, tri, [mvp], [torch.zeros(res, res, 1, device=dev)], (res, res))
    with torch.no_grad():
        t = deformer.renderer.render([mvp], moved, tri, mg.normals(moved, geo)[1], (res, res), ["mask", "normal"],
                                     topology=geo.topology)[0]
        g0 = deformer.renderer.render([mvp], v, tri, mg.normals(v, geo)[1], (res, res), CHANNELS, topology=geo.topology)[0]
    deformer.target_masks = [t["mask"]]
    normal_map = (0.5 * (t["normal"] @ R.T @ torch.diag(torch.tensor([1.0, -1.0, -1.0], device=dev)).T + 1)).contiguous()
    rgb = torch.from_numpy(rng.uniform(0, 1, (res, res, 3)).astype(np.float32)).to(dev)
    view = ml.View(normal_map, t["mask"], R, center, rgb)
    shader = ns.NeuralShader(device=dev, seed=0)
    reference = TorchShader(shader)
    out = {}

    # the stages of one view through the entries
    H = W = res
    capacity = H * W
    cap, rows = C.c_int64(capacity), ns.rows_of(capacity)
    index = torch.empty(capacity, dtype=torch.int32, device=dev)
    counters = torch.empty(4, dtype=torch.int32, device=dev)
    act = torch.empty(rows * ns.ACT_WIDTH, dtype=torch.bfloat16, device=dev)
    dz = torch.empty(rows * ns.DZ_WIDTH, dtype=torch.bfloat16, device=dev)
    logits = torch.empty(rows, 3, device=dev)
    dfeat, dextra = torch.empty(rows, 32, device=dev), torch.empty(rows, 32, device=dev)
    loss, dloss = torch.empty(1, device=dev), torch.ones(1, device=dev)
    work = ns.workspace(capacity, dev)
    select_work = scratch(_native.lib().gd_shader_select_scratch_bytes(H * W), dev)
    camera = ml.camera_block(view)
    position, normal, mask, view_mask = g0["position"].contiguous(), g0["normal"].contiguous(), \
        g0["mask"][..., 0].contiguous(), view.mask[..., 0].contiguous()
    dposition, dnormal = torch.empty_like(position), torch.empty_like(position)

    def select_features():
        launch("gd_shader_select", dev, H, W, normal, position, mask, view_mask, camera, C.c_float(PERCENTAGE), C.c_uint32(0),
               C.c_uint32(0), cap, index, counters, select_work)
        launch("gd_shader_features", dev, H, W, position, normal, camera, cap, index, counters, act)

    def l1():
        launch("gd_shader_l1_forward", dev, H, W, cap, index, counters, logits, rgb, loss, work)
        launch("gd_shader_l1_backward", dev, H, W, cap, index, counters, logits, rgb, dloss, dz, None)

    def backward():
        for l in range(ns.LAYERS - 1, -1, -1):
            launch("gd_shader_backward_weight_layer", dev, l, cap, counters, act, dz, shader.flat_grad, work)
            launch("gd_shader_backward_input_layer", dev, l, cap, counters, shader.packed_t, act, dz, dfeat, dextra)
        launch("gd_shader_features_backward", dev, H, W, position, camera, cap, index, counters, dfeat, dextra, dposition,
               dnormal)

    select_features()
    shader.forward_layers(capacity, counters, act, logits)
    l1()
    count = int(counters[0])
    out["points"] = count
    g_ref = {"position": g0["position"].clone().requires_grad_(True), "normal": g0["normal"].clone().requires_grad_(True),
             "mask": g0["mask"]}
    gathered = [t.detach() for t in torch_gather(view, g_ref, PERCENTAGE)]
    gathered[0].requires_grad_(True)
    gathered[1].requires_grad_(True)
    colour = reference(*gathered[:3])
    torch_loss = F.l1_loss(colour, gathered[3])
    out["select_features"] = pair(select_features, lambda: torch_gather(view, g_ref, PERCENTAGE), args.iters)
    out["forward_products"] = pair(lambda: shader.forward_layers(capacity, counters, act, logits),
                                   lambda: reference(*gathered[:3]), args.iters)
    out["l1"] = pair(l1, lambda: torch.autograd.grad(F.l1_loss(colour, gathered[3]), colour, retain_graph=True), args.iters)
    out["backward"] = pair(backward, lambda: torch_loss.backward(retain_graph=True), args.iters)
    out["forward_tflops"] = 2.0 * MACS * count / out["forward_products"]["hip_us"] * 1e-6
    out["backward_tflops"] = 4.0 * MACS * count / out["backward"]["hip_us"] * 1e-6
    out["pack_us"] = median_us(shader.pack, args.iters)
    out["bytes_per_point"] = {"activations": 2 * ns.ACT_WIDTH, "dz": 2 * ns.DZ_WIDTH, "logits_dfeat_dextra": 12 + 256}

    # the whole loss of one view, forward and backward, through the public function
    g_hip = {"position": g0["position"].clone().requires_grad_(True), "normal": g0["normal"].clone().requires_grad_(True),
             "mask": g0["mask"]}

    def hip_loss():
        ml.shading_loss([view], [g_hip], shader, PERCENTAGE).backward()

    def ref_loss():
        torch_shading(view, g_ref, reference, PERCENTAGE).backward()

    out["shading_loss_forward_backward"] = pair(hip_loss, ref_loss, args.iters)
    del act, dz, dfeat, dextra, index, logits

    # one second-stage iteration, one view: without a shader, with it, and with the torch composition as extra_loss
    def second_stage(with_shader):
        d = Deformer(v, tri, [mvp], [t["mask"]], (res, res))
        for _ in range(3):
            d.step([0])
        if with_shader:
            d.begin_second_stage([normal_map], [R], [center], target_rgbs=[rgb], shader=ns.NeuralShader(device=dev, seed=0))
        else:
            d.begin_second_stage([normal_map], [R], [center])
        return d

    plain, shaded, composed = second_stage(False), second_stage(True), second_stage(False)
    optimizer = torch.optim.Adam(reference.parameters(), lr=1e-3)
    torch_view = ml.View(normal_map, t["mask"], R, center, rgb)

    def torch_step():
        optimizer.zero_grad()
        composed.step_second([0], extra_loss=lambda views, gbuffers: torch_shading(torch_view, gbuffers[0], reference, PERCENTAGE))
        optimizer.step()

    out["step_second_without_shader_us"] = median_us(lambda: plain.step_second([0]), args.iters)
    out["step_second"] = pair(lambda: shaded.step_second([0]), torch_step, args.iters)
    out["hip_step_trips_sync_debug"] = trips_sync_debug(lambda: shaded.step_second([0]))
    out["torch_step_trips_sync_debug"] = trips_sync_debug(torch_step)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[1024, 512])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--nu", type=int, default=192)
    ap.add_argument("--nv", type=int, default=130)
    args = ap.parse_args()
    res = {"multiply_adds_per_point": MACS, "shading_percentage": PERCENTAGE}
    for r in args.res:
        res[str(r)] = one_resolution(r, args, "cuda:0")
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
