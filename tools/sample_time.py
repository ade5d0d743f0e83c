"""Time the texture sampling of ``garmentdreamer_amd/texture_sample.py`` (include/gd_sample.h) on one GPU: 1024 x 1024
pixels against a 2048 x 2048 three-channel albedo.

    python tools/sample_time.py [--pixels 1024] [--texture 2048] [--runs 5]

Prints one JSON line of milliseconds per call, each step timed with events around 20 back-to-back calls after a warm-up,
best of ``runs``: ``build_mipmaps``; per filter mode the forward kernel, the whole ``texture()`` call and the backward (with
its phases: items, the stable sort, reduce and fold) on a render-like uv field (a rotated, slowly varying map at about two
texels per pixel, so the mip filters blend levels 0-2); ``render_mesh`` of a pleated tube with a chart atlas (a call that
builds its topology on the host and inverts the pose, so it is host time as much as kernels); and, as the yardstick for
the forward, a plain device-to-device copy of the bytes it must touch whatever it reads of the texture (``out`` + ``uv`` +
``uv_da``).  A record, not a criterion: the operations are new, so there is no earlier figure, and nvdiffrast is not
available to compare with."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from garmentdreamer_amd import _native  # noqa: E402
from garmentdreamer_amd import texture_atlas as ta  # noqa: E402
from garmentdreamer_amd import texture_sample as ts  # noqa: E402
from garmentdreamer_amd._launch import launch  # noqa: E402
from tools.atlas_time import pleated_tube  # noqa: E402


def timed(fn, runs, reps=20):
    """best milliseconds per call: ``reps`` calls between two events (one call is a window of tens of microseconds, which
    measures the events as much as the kernel), after a warm-up call, best of ``runs`` windows"""
    fn()
    best = None
    for _ in range(runs):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        ms = start.elapsed_time(stop) / reps
        best = ms if best is None else min(best, ms)
    return round(best, 4)


def uv_field(n, texels_per_pixel, res, dev):
    """uv [n,n,2] and uv_da [n,n,4] of a rotated map with a gentle wave: about ``texels_per_pixel`` texels per pixel"""
    y, x = torch.meshgrid(torch.arange(n, device=dev, dtype=torch.float32), torch.arange(n, device=dev, dtype=torch.float32),
                          indexing="ij")
    s = texels_per_pixel / res
    c, sn = np.cos(0.3), np.sin(0.3)
    wave = 0.02 * torch.sin(x * 0.01)
    u = s * (c * x - sn * y) + wave
    v = s * (sn * x + c * y)
    dudx = s * c + 0.02 * 0.01 * torch.cos(x * 0.01)
    da = torch.stack((dudx, torch.full_like(x, -s * sn), torch.full_like(x, s * sn), torch.full_like(x, s * c)), dim=-1)
    return torch.stack((u, v), dim=-1).contiguous(), da.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pixels", type=int, default=1024)
    ap.add_argument("--texture", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    n, res, C = args.pixels, args.texture, 3
    torch.manual_seed(0)
    tex = torch.rand(res, res, C, device=dev)
    uv, da = uv_field(n, 2.0, res, dev)
    N = n * n
    ms = {"build_mipmaps": timed(lambda: ts.build_mipmaps(tex), args.runs)}
    mip = ts.build_mipmaps(tex)
    level0 = ts.build_mipmaps(tex, 0)
    flat_uv, flat_da = uv.view(N, 2), da.view(N, 4)
    dout = torch.rand(N, C, device=dev)
    for name, fid in _native.SAMPLE_FILTERS.items():
        pyramid = mip if name in ts.MIP_FILTERS else level0
        out = torch.empty(N, C, device=dev)
        lay = pyramid.layout
        ms["forward " + name] = timed(lambda: launch("gd_sample_texture_forward", dev, N, C, fid, 0, lay, pyramid.buffer,
                                                     flat_uv, flat_da, out), args.runs)
        ms["texture() " + name] = timed(lambda: ts.texture(None, uv, da, mip=pyramid, filter_mode=name), args.runs)
        taps = _native.lib().gd_sample_taps(fid)
        keys = torch.empty(N * taps, dtype=torch.int64, device=dev)
        vals = torch.empty(N * taps, C, device=dev)
        items = lambda: launch("gd_sample_texture_items", dev, N, C, fid, 0, lay, flat_uv, flat_da, dout, keys, vals)  # noqa: E731
        ms["backward " + name + ": items"] = timed(items, args.runs)
        ms["backward " + name + ": sort"] = timed(lambda: torch.sort(keys, stable=True), args.runs)
        skeys, order = torch.sort(keys, stable=True)
        gpyr = torch.zeros(lay.offset[lay.levels], 4, device=dev)
        dtex = torch.zeros_like(tex)
        ms["backward " + name + ": reduce"] = timed(
            lambda: launch("gd_sample_texture_reduce", dev, N * taps, C, lay, skeys, order, vals, gpyr), args.runs)
        ms["backward " + name + ": fold"] = timed(lambda: launch("gd_sample_texture_fold", dev, C, lay, gpyr.clone(), dtex),
                                                  args.runs)
        ms["backward " + name] = timed(lambda: ts.texture_backward(lay, C, flat_uv, flat_da, dout, fid, 0, dtex), args.runs)
        del keys, vals, skeys, order, gpyr, dtex
    # the yardstick: the bytes the forward touches besides the texture, moved once
    src = torch.empty(N * (C + 2 + 4), device=dev)
    dst = torch.empty_like(src)
    ms["copy of out + uv + uv_da"] = timed(lambda: dst.copy_(src), args.runs)
    ms["copy of out + uv"] = timed(lambda: dst[:N * (C + 2)].copy_(src[:N * (C + 2)]), args.runs)

    v, f = (torch.from_numpy(a).to(dev) for a in pleated_tube(200, 100))
    vt, ft, info = ta.chart_atlas(v, f, res)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], dtype=np.float32)     # camera on +x, z up
    pose[:3, 3] = (1.6, 0.0, 0.5)
    y = np.tan(0.75 / 2)
    proj = np.array([[1 / y, 0, 0, 0], [0, -1 / y, 0, 0], [0, 0, -100.01 / 99.99, -2.0 / 99.99], [0, 0, -1, 0]], dtype=np.float32)
    vn = ts._vertex_normals(v, f.to(torch.int32))
    for name in ("linear", "linear-mipmap-linear"):
        ms["render_mesh " + name] = timed(
            lambda: ts.render_mesh(v, f, vt, ft, mip if name in ts.MIP_FILTERS else level0, vn, pose, proj, n, n,
                                   texture_filter=name, boundary_mode="clamp"), args.runs, reps=3)
    out = ts.render_mesh(v, f, vt, ft, mip, vn, pose, proj, n, n, boundary_mode="clamp")
    print(json.dumps({"pixels": [n, n], "texture": [res, res, C], "pyramid_mib": round(mip.buffer.numel() * 4 / 2 ** 20, 1),
                      "touched_mib": round(N * (C + 2 + 4) * 4 / 2 ** 20, 1), "covered": round(float((out["alpha"] > 0).float().mean()), 3),
                      "faces": int(f.shape[0]), "ms": ms}))


if __name__ == "__main__":
    main()
