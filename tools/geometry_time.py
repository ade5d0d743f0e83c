"""Time what the NeTF stage with free geometry adds, on one GPU: the texture field's fused backward with and without the
gradient to the positions (include/gd_texture_position.h), both grid-gradient paths, production layout (16 levels, 2^19
entries), at N = res^2 uniform points; and one ``DeformableNeTFRenderer`` iteration (render, backward, optimizer step,
``zero_grad``) at res x res next to the ``NeTFRenderer`` iteration on the same mesh with the geometry fixed.

    python tools/geometry_time.py [--res 512] [--iters 30] [--nu 192] [--nv 130] [--parent-lib libgd_raster.so]
                                  [--limit 120]

Prints one JSON line.  One process; every GPU step runs under a time limit of its own (``--limit`` seconds: a watchdog
thread ends the process with status 124 and says which step it was, so a step that hangs starts nothing after it).  The
kernel columns are timed as in tools/texture_sorted_time.py: HIP-event intervals on the current stream around the C
entries, every buffer allocated beforehand, 5 warm-ups, medians of ``--iters`` runs, the columns ALTERNATED.
``--parent-lib``: a build of the parent commit, whose ``gd_texture_field_backward`` is timed as a further alternated
column on the same machine in the same run (``field_backward_kernel`` became a wrapper of a shared body).
``traffic`` is what the definitions imply per fused backward, not a counter: the float2 gathers of the forward's
recomputation, the gathers ``dx`` adds, and the float atomics of ``dgrid``."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
from contextlib import contextmanager

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from garmentdreamer_amd import _native  # noqa: E402
from garmentdreamer_amd import mesh_render as mr  # noqa: E402
from garmentdreamer_amd import netf_geometry as ng  # noqa: E402
from garmentdreamer_amd import texture_field as tf  # noqa: E402
from garmentdreamer_amd._launch import launch  # noqa: E402
from mesh_losses_time import trips_sync_debug  # noqa: E402
from mesh_render_time import look_at, median_us, tube  # noqa: E402
from texture_sorted_time import alternated_us, parent_field_backward  # noqa: E402

DEV = "cuda:0"


@contextmanager
def step_limit(name, seconds):
    """the process ends with status 124 if the step has not finished after ``seconds`` (from a thread: a wait inside the
    HIP runtime does not return to the interpreter, so a signal handler would never run)"""
    def expired():
        sys.stderr.write(f"geometry_time: step '{name}' exceeded its limit of {seconds} s\n")
        sys.stderr.flush()
        os._exit(124)
    timer = threading.Timer(seconds, expired)
    timer.daemon = True
    timer.start()
    try:
        yield
        torch.cuda.synchronize()
    finally:
        timer.cancel()


def kernel_columns(n, fld, parent):
    L = _native.lib()
    s = fld.encoder.layout.struct()
    grid = fld.encoder.params.detach()
    w1, b1, w2, b2 = (p.detach() for p in fld.mlp.parameters())
    x = torch.rand(n, 3, device=DEV) * 2 - 1
    with torch.no_grad():
        color = fld(x).contiguous()
    dcolor, denc = torch.rand(n, 3, device=DEV), torch.rand(n, 32, device=DEV)
    grads = [torch.zeros_like(t) for t in (grid, w1, b1, w2, b2)]
    denc_out, dx = torch.empty(n, 32, device=DEV), torch.empty(n, 3, device=DEV)
    slab = torch.empty(max(L.gd_texture_field_backward_scratch_bytes(n), 1), dtype=torch.uint8, device=DEV)
    sort = torch.empty(max(L.gd_texture_sorted_scratch_bytes(n, s), 1), dtype=torch.uint8, device=DEV)
    head = (DEV, n, x, None, grid, s, w1, b1, w2, b2, color, dcolor, *grads)
    cols = {
        "fused_backward_atomic": lambda: launch("gd_texture_field_backward", *head, slab),
        "fused_backward_atomic_dx": lambda: launch("gd_texture_field_backward_pos", *head, dx, slab),
        "fused_backward_sorted": lambda: launch("gd_texture_field_backward_sorted", *head, denc_out, slab, sort),
        "fused_backward_sorted_dx": lambda: launch("gd_texture_field_backward_sorted_pos", *head, denc_out, dx, slab, sort),
        "encode_backward_dx_alone": lambda: launch("gd_texture_encode_backward_pos", DEV, n, x, None, grid, s, denc, dx),
    }
    if parent is not None:
        stream = torch.cuda.current_stream(DEV).cuda_stream
        args = [t.data_ptr() if isinstance(t, torch.Tensor) else t for t in head[2:]] + [slab.data_ptr()]
        cols["fused_backward_atomic_parent_build"] = lambda: parent(stream, n, *args)
    return cols


def iterations(res, nu, nv):
    """(free geometry, fixed geometry): one training iteration each on the same tube, field and target"""
    v, tri, vn = (torch.from_numpy(a).to(DEV) for a in tube(nu, nv))
    pose, proj = look_at((1.5, 0.4, 1.45)), mr.perspective(0.75)
    target = torch.rand(res, res, 3, device=DEV)

    def make(free):
        fld = tf.TextureField(generator=torch.Generator().manual_seed(0), position_gradient=free).to(DEV)
        renderer = ng.DeformableNeTFRenderer(v, tri, fld) if free else tf.NeTFRenderer(v, tri, vn, fld)
        opt = renderer.optimizer() if free else fld.optimizer()

        def run():
            loss = ((renderer.render(pose, proj, res, res)["image"] - target) ** 2).mean()
            loss.backward()
            opt.step()
            opt.zero_grad()
            return loss.detach()
        return run
    return make(True), make(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--nu", type=int, default=192)
    ap.add_argument("--nv", type=int, default=130)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--limit", type=float, default=120.0)
    args = ap.parse_args()
    torch.manual_seed(0)
    n = args.res * args.res
    res = {"points": n, "iters": args.iters, "alternated": True}
    with step_limit("set-up", args.limit):
        fld = tf.TextureField(generator=torch.Generator().manual_seed(0)).to(DEV)
        parent = parent_field_backward(args.parent_lib) if args.parent_lib else None
        cols = kernel_columns(n, fld, parent)
    with step_limit("kernels", args.limit):
        res["kernels_us"] = alternated_us(cols, args.iters)
    levels, corners = fld.encoder.layout.num_levels, 8
    res["traffic"] = {"gathers_forward_recompute": n * levels * corners, "gathers_dx": n * levels * corners,
                      "gather_bytes_each": 8, "float_atomics_dgrid": n * levels * corners * 2,
                      "dx_bytes_written": 12 * n}
    k = res["kernels_us"]
    res["dx_costs_us"] = {"atomic": round(k["fused_backward_atomic_dx"] - k["fused_backward_atomic"], 1),
                          "sorted": round(k["fused_backward_sorted_dx"] - k["fused_backward_sorted"], 1)}
    with step_limit("iteration set-up", args.limit):
        free, fixed = iterations(args.res, args.nu, args.nv)
    with step_limit("iteration, free geometry", args.limit):
        res["iteration_free_geometry_us"] = median_us(free, args.iters)
    with step_limit("iteration, fixed geometry", args.limit):
        res["iteration_fixed_geometry_us"] = median_us(fixed, args.iters)
    with step_limit("sync debug", args.limit):
        res["free_geometry_trips_sync_debug"] = trips_sync_debug(free)
    res["triangles"] = 2 * args.nu * args.nv
    print(json.dumps(res))


if __name__ == "__main__":
    main()
