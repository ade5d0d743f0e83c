"""Time ``views.read_views`` (garmentdreamer_amd/views.py, include/gd_views.h) on N synthetic views written with mixed row
filters, next to the only reader the package had before: ``export.load_image_rgb`` per file plus the torch statement of the
unpack and the upload of its float images.

    python tools/views_time.py [--views 8] [--side 1024] [--workers 8] [--baseline-views 2] [--repeats 3]

Writes the capture into a temporary directory (two RGBA PNGs per view, a seeded random filter type 0-4 per row over a
smooth image with noise, and ``cameras.json``), then prints one JSON line: ``read_views_s`` (the best of ``--repeats`` whole
calls, nothing waited for inside), ``split_s`` (one more call with ``timings=``: ``inflate``, ``upload``, ``unfilter``,
``unpack``, the GPU waited for after each phase), ``unfilter_kernel_ms`` and ``unpack_kernel_ms`` (HIP-event medians of the
launches alone, all views in one batch), and ``baseline_s_per_view`` / ``baseline_s`` (``--baseline-views`` views read the old
way, scaled to N)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from garmentdreamer_amd import export, views  # noqa: E402
from tests import views_reference as vref  # noqa: E402


def synthetic(side, seed):
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    smooth = np.stack([(x + y) // 8, (2 * x + y) // 16, (x + 3 * y) // 16, 255 * ((x - side / 2) ** 2 + (y - side / 2) ** 2
                                                                                   < (0.4 * side) ** 2)], axis=-1)
    return ((smooth + rng.integers(0, 3, size=smooth.shape)) % 256).astype(np.uint8)


def write_capture(folder, n, side):
    records = [export.camera_info_entry(vref.rigid_c2w(i + 1), i, side, side, 0.6) for i in range(n)]
    export.save_cameras_json(os.path.join(folder, views.CAMERAS_FILE), records)
    for k, sub in enumerate((views.NORMAL_DIRECTORY, views.RGB_DIRECTORY)):
        os.makedirs(os.path.join(folder, sub))
        for i in range(n):
            vref.write_png(os.path.join(folder, sub, f"{i}.png"), synthetic(side, 2 * i + k), vref.kinds_for(side, "mixed", 2 * i + k))


def event_ms(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def baseline_view(folder, i, dev):
    """one view through the reader of before: the byte-wise Python unfilter, View.load's arithmetic in torch, three uploads"""
    normal_rgba = export.load_image_rgb(os.path.join(folder, views.NORMAL_DIRECTORY, f"{i}.png"))
    rgba = export.load_image_rgb(os.path.join(folder, views.RGB_DIRECTORY, f"{i}.png"))
    return [t.to(dev) for t in vref.unpack_torch(normal_rgba, rgba)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--baseline-views", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda:0"
    res = {"views": args.views, "side": args.side, "workers": args.workers}
    with tempfile.TemporaryDirectory() as folder:
        write_capture(folder, args.views, args.side)
        res["file_bytes"] = sum(os.path.getsize(os.path.join(folder, sub, f)) for sub in (views.NORMAL_DIRECTORY, views.RGB_DIRECTORY)
                                for f in os.listdir(os.path.join(folder, sub)))
        views.read_views(folder, device=dev, workers=args.workers)        # warms the allocators and the page cache
        whole = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = views.read_views(folder, device=dev, workers=args.workers)
            torch.cuda.synchronize()
            whole.append(time.perf_counter() - t0)
        res["read_views_s"] = min(whole)
        split = {}
        views.read_views(folder, device=dev, workers=args.workers, timings=split)
        res["split_s"] = split
        paths = [os.path.join(folder, views.RGB_DIRECTORY, f"{i}.png") for i in range(args.views)]
        rows = np.stack([views._inflate(p)[1] for p in paths])
        filtered = torch.from_numpy(rows).to(dev).reshape(-1)
        res["unfilter_kernel_ms"] = event_ms(lambda: views.png_unfilter(filtered, args.views, args.side, args.side, 4), 5)
        image = views.png_unfilter(filtered, args.views, args.side, args.side, 4)[0].contiguous()
        res["unpack_kernel_ms"] = event_ms(lambda: views.unpack_view(image, image), 5)
        n = max(1, min(args.baseline_views, args.views))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            old = baseline_view(folder, i, dev)
        torch.cuda.synchronize()
        res["baseline_s_per_view"] = (time.perf_counter() - t0) / n
        res["baseline_s"] = res["baseline_s_per_view"] * args.views
        res["equal"] = all(torch.equal(a, b) for a, b in zip((got[n - 1].normal, got[n - 1].mask, got[n - 1].rgb), old))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
