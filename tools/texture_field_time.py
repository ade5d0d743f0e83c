"""Time the NeTF texture field (garmentdreamer_amd/texture_field.py, include/gd_texture.h) on one GPU, next to the same
definition written as a torch composition on the same GPU (integer index arithmetic, a gather, ``index_add_`` through
autograd, two ``nn.Linear``), on the production layout (16 levels, 2^19 entries, 45.7 MB): at N = 262 144 uniform points
and at N = the pixels of the 49 920-triangle ``tube(192, 130)`` at 512 x 512 with its coverage as the mask.

    python tools/texture_field_time.py [--res 512] [--iters 50] [--points 262144]

Prints one JSON line.  The method is tools/mesh_render_time.py's: medians of HIP-event intervals on the current stream
around the Python calls (autograd and allocations included), 5 warm-up runs.  A backward is timed on a retained graph and
adds into the optimizer's flat gradient buffer (this package) or into ``.grad`` (the composition).  The columns are timed
one after the other, not alternated.

``scatter`` isolates the gradient to the grid (``gd_texture_encode_backward``, 1 024 bytes of float atomics per point): the
production layout; the same with levels 0-2 removed; and the same with levels 0-2 replaced by three more 2^19-entry hashed
levels (equal bytes, spread over a table)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from garmentdreamer_amd import mesh_render as mr  # noqa: E402
from garmentdreamer_amd import texture_field as tf  # noqa: E402
from mesh_render_time import look_at, median_us, tube  # noqa: E402

M32 = 0xFFFFFFFF
CORNERS = [[(i >> d) & 1 for d in range(3)] for i in range(8)]


def torch_encode(x, grid, layout, mask=None):
    """include/gd_texture.h's encoding, one level at a time, the eight corners of a level at once"""
    u = (x + 1) * 0.5
    table = grid.view(-1, 2)
    delta = torch.tensor(CORNERS, device=x.device)                              # [8,3]
    cols = []
    for l in range(layout.num_levels):
        p = u * float(layout.scale[l]) + 0.5
        fl = torch.floor(p)
        w = (p - fl)[:, None, :]                                                # [N,1,3]
        g = (fl.long()[:, None, :] + delta) & M32                               # [N,8,3]
        res, size = int(layout.res[l]), int(layout.size[l])
        if layout.dense[l]:
            idx = (g[..., 0] + g[..., 1] * res + g[..., 2] * (res * res)) & M32
        else:
            idx = g[..., 0] ^ ((g[..., 1] * 2654435761) & M32) ^ ((g[..., 2] * 805459861) & M32)
        idx = idx % size + int(layout.offset[l])
        wt = torch.where(delta.bool(), w, 1 - w).prod(dim=-1)                   # [N,8]
        cols.append((wt[..., None] * table[idx]).sum(dim=1))
    enc = torch.cat(cols, dim=1)
    return enc if mask is None else enc * mask[:, None]


class TorchField(torch.nn.Module):
    def __init__(self, fld):
        super().__init__()
        self.layout = fld.encoder.layout
        self.grid = torch.nn.Parameter(fld.encoder.params.detach().clone())
        self.l1, self.l2 = torch.nn.Linear(32, 32), torch.nn.Linear(32, 3)
        self.to(self.grid.device)
        with torch.no_grad():
            for dst, src in zip(list(self.l1.parameters()) + list(self.l2.parameters()), fld.mlp.parameters()):
                dst.copy_(src)

    def forward(self, x, mask=None):
        m = None if mask is None else mask.float()
        color = torch.sigmoid(self.l2(torch.relu(self.l1(torch_encode(x, self.grid, self.layout, m)))))
        return color if m is None else color * m[:, None]


def pair(hip, ref, iters):
    out = {"hip_us": median_us(hip, iters)}
    try:
        out["torch_us"] = median_us(ref, iters)
    except Exception as e:   # the composition, not this package: report it and go on
        out["torch_us"] = None
        out["torch_error"] = repr(e)[:200]
    return out


def sub_layout(layout, keep):
    scale, res, size = layout.scale[keep], layout.res[keep], layout.size[keep]
    offset = np.concatenate(([0], np.cumsum(size))).astype(np.int64)
    return tf.GridLayout(len(keep), scale, res, size, offset, res ** 3 <= size)


def time_points(name, x, mask, fld, ref, iters, report):
    n = x.shape[0]
    dcolor = torch.rand(n, 3, device=x.device)
    denc = torch.rand(n, 32, device=x.device)

    def retained(fn):
        out = fn()
        return lambda g: (lambda: out.backward(g, retain_graph=True))

    hip_enc = retained(lambda: fld.encoder(x, mask=mask))
    ref_enc = retained(lambda: torch_encode(x, ref.grid, ref.layout, None if mask is None else mask.float()))
    hip_fused = retained(lambda: fld(x, mask))
    hip_unfused = retained(lambda: fld.unfused(x, mask))
    ref_field = retained(lambda: ref(x, mask))
    valid = n if mask is None else int(mask.sum())
    out = {"points": n, "valid_points": valid}
    with torch.no_grad():
        out["encode_forward"] = pair(lambda: fld.encoder(x, mask=mask),
                                     lambda: torch_encode(x, ref.grid, ref.layout, None if mask is None else mask.float()),
                                     iters)
        out["fused_forward"] = pair(lambda: fld(x, mask), lambda: ref(x, mask), iters)
        out["unfused_forward"] = {"hip_us": median_us(lambda: fld.unfused(x, mask), iters)}
    out["encode_backward"] = pair(hip_enc(denc), ref_enc(denc), iters)
    out["fused_backward"] = pair(hip_fused(dcolor), ref_field(dcolor), iters)
    out["unfused_backward"] = {"hip_us": median_us(hip_unfused(dcolor), iters)}
    out["atomic_bytes"] = valid * 1024
    out["encode_backward_atomic_TBps"] = round(valid * 1024 / out["encode_backward"]["hip_us"] / 1e6, 4)
    report[name] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--points", type=int, default=262144)
    ap.add_argument("--nu", type=int, default=192)
    ap.add_argument("--nv", type=int, default=130)
    args = ap.parse_args()
    dev = "cuda:0"
    torch.manual_seed(0)
    fld = tf.TextureField(generator=torch.Generator().manual_seed(0)).to(dev)
    ref = TorchField(fld)
    opt = fld.optimizer()
    ref_opt = torch.optim.Adam([{"params": [ref.grid], "lr": 0.01},
                                {"params": list(ref.l1.parameters()) + list(ref.l2.parameters()), "lr": 0.001}])
    res = {"layout_MB": round(fld.encoder.layout.num_params * 4 / 1e6, 1), "iters": args.iters}

    x = torch.rand(args.points, 3, device=dev) * 2 - 1
    time_points("uniform", x, None, fld, ref, args.iters, res)

    v, tri, vn = (torch.from_numpy(a).to(dev) for a in tube(args.nu, args.nv))
    pose, proj = look_at((1.5, 0.4, 1.45)), mr.perspective(0.75)
    h = w = args.res
    netf = tf.NeTFRenderer(v, tri, vn, fld)
    mesh = mr.MeshRenderer(v, tri, vn, ref)
    seen = {}

    def keep(xyz, mask):
        seen["x"], seen["mask"] = xyz.detach().clone(), mask.detach().clone().view(torch.uint8)
        return fld(xyz, mask)

    netf.texture_fn = keep
    with torch.no_grad():
        netf.render(pose, proj, h, w)
    netf.texture_fn = fld
    time_points("tube_pixels", seen["x"], seen["mask"], fld, ref, args.iters, res)
    res["tube_pixels"]["triangles"], res["tube_pixels"]["resolution"] = int(tri.shape[0]), h

    # the optimizer: one launch over the flat buffer against torch.optim.Adam over the same two groups
    (ref(x[:4096]) ** 2).mean().backward()
    res["optimizer_step"] = pair(opt.step, ref_opt.step, args.iters)

    # one iteration of the stage without the guidance: render, image loss, backward, step
    target = torch.rand(h, w, 3, device=dev)

    def hip_iteration():
        opt.zero_grad()
        ((netf.render(pose, proj, h, w)["image"] - target) ** 2).mean().backward()
        opt.step()

    def torch_iteration():
        ref_opt.zero_grad(set_to_none=True)
        ((mesh.render(pose, proj, h, w)["image"] - target) ** 2).mean().backward()
        ref_opt.step()

    res["render_backward_step"] = pair(hip_iteration, torch_iteration, args.iters)

    # what the scatter costs, and what its three smallest levels cost
    layout = fld.encoder.layout
    denc = torch.rand(args.points, 32, device=dev)

    def scatter_us(lay, d):
        grid = torch.zeros(lay.num_params, device=dev, requires_grad=True)
        grid._gd_grad_sink = torch.zeros(lay.num_params, device=dev)
        enc = tf.encode(x, grid, lay)
        return median_us(lambda: enc.backward(d, retain_graph=True), args.iters)

    full = scatter_us(layout, denc)
    without = scatter_us(sub_layout(layout, list(range(3, 16))), denc[:, 6:].contiguous())
    spread = scatter_us(sub_layout(layout, [15, 15, 15] + list(range(3, 16))), denc)
    res["scatter"] = {"points": args.points, "production_us": full, "without_levels_0_2_us": without,
                      "levels_0_2_as_hashed_us": spread, "production_atomic_TBps": round(args.points * 1024 / full / 1e6, 4),
                      "spread_atomic_TBps": round(args.points * 1024 / spread / 1e6, 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
