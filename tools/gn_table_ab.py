#!/usr/bin/env python
"""Bit-equality of the GroupNorm-in-the-loader convolutions between two builds of libgd_nn.so.

    python tools/gn_table_ab.py <libgd_nn.so A> <libgd_nn.so B>

``nn_ops.use_library`` takes one library per process, so each build runs in a child process of its own (this file with
``--child``), on the same seeded inputs, and saves every output (the large ones as the SHA-256 of their bytes); the parent
process loads both sets and asserts ``torch.equal`` (equal digests) case by case.  Entries: gd_nn_conv3x3_wide_gn_forward, gd_nn_conv3x3_gn_forward,
gd_nn_conv3x3_gn_forward_stats, gd_nn_conv3x3_wino_gn_forward (the persistent streaming kernel has no GroupNorm entry:
every GroupNorm launch of the patch path runs conv3x3_gn_patch_kernel).  Shapes: those of
tests/test_conv_gn_table_gpu.py, and the GroupNorm-fused launches of the VAE encoder in one 8-view SDS step (four
128 -> 128 @512^2, one 128 -> 256 and three 256 -> 256 @256^2; with and without residual), outputs and statistics.  The
last field of a case tells whether the GroupNorm loader is on: the plain wide-tile and Winograd entries run the same
epilogues (PLAIN below).
"""
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, ".")
import torch  # noqa: E402

CL = torch.channels_last
# kind, N, Cin, Cout, H, W, residual, statistics, silu
SMALL = [(k, 2, c, 64, 20, 40, 0, 0, 1) for k, cs in (("wide", (64, 128, 160, 320)), ("wino", (64, 128, 160, 320)),
                                                        ("patch", (64, 128, 320))) for c in cs] + \
        [("wide", n, 64, 64, 192, 256, 0, 0, 1) for n in (3, 5)] + \
        [(k, n, 64, 64, 160, 160, 0, 0, 1) for k in ("patch", "wino") for n in (3, 5)] + \
        [(k, 2, 128, 136, 36, 40, 1, 1, s) for k in ("wide", "patch", "wino") for s in (0, 1)]
VAE = [(k, 8, 128, 128, 512, 512, r, 1, 1) for k in ("wide", "patch", "wino") for r in (1, 0)] + \
      [(k, 8, 128, 256, 256, 256, 0, 1, 1) for k in ("patch", "wino")] + \
      [(k, 8, 256, 256, 256, 256, r, 1, 1) for k in ("patch", "wino") for r in (1, 0)]
# the same entries' plain twins (no GroupNorm in the loader), which share the epilogues: ragged test shapes, and the plain
# conv2 launches of the step that carry a residual (VAE 128^2 / 64^2 levels, UNet levels at 2 x 8 latents)
PLAIN = [(k, 2, 96, 320, 20, 40, r, 1, 0) for k in ("wide", "wino") for r in (1, 0)] + \
        [("wino", n, c, c, hw, hw, r, 0, 0) for (n, c, hw) in ((8, 512, 128), (8, 512, 64), (16, 320, 64), (16, 640, 32),
                                                                 (16, 1280, 16)) for r in (1, 0)]
CASES = [c + (1,) for c in SMALL + VAE] + [c + (0,) for c in PLAIN]


def child(lib_path, out_dir):
    from garmentdreamer_amd import nn_ops
    nn_ops.use_library(lib_path)
    L = nn_ops.lib()
    dev = "cuda:0"
    for i, (kind, N, Cin, Cout, H, W, res, stats, silu, gn) in enumerate(CASES):
        g = torch.Generator(dev).manual_seed(1000 + i)
        x = torch.randn(N, Cin, H, W, device=dev, generator=g) * 1.5 + 0.3
        n = torch.arange(N, device=dev, dtype=torch.float32).view(N, 1, 1, 1)
        x = (x * (n + 1) + n).to(torch.bfloat16).contiguous(memory_format=CL)
        w = (torch.randn(Cout, Cin, 3, 3, device=dev, generator=g) / (3 * Cin ** 0.5)).to(torch.bfloat16).contiguous(memory_format=CL)
        b = torch.randn(Cout, device=dev, generator=g).to(torch.bfloat16)
        r = torch.randn(N, Cout, H, W, device=dev, generator=g).to(torch.bfloat16).contiguous(memory_format=CL) if res else None
        gw = (torch.randn(Cin, device=dev, generator=g) * 0.5 + 1).to(torch.bfloat16)
        gb = (torch.randn(Cin, device=dev, generator=g) * 0.5).to(torch.bfloat16)
        xg = x.float().reshape(N, 32, -1)
        mr = torch.stack([xg.mean(-1), (xg.var(-1, unbiased=False) + 1e-6).rsqrt()], -1).reshape(-1).contiguous()
        del xg
        rows = ((H + 15) // 16) * ((W + 15) // 16) * 8
        part = torch.zeros(N * (Cout // 4) * rows * 2, dtype=torch.float32, device=dev) if stats else None
        out = {}
        with torch.no_grad():
            out["y"] = nn_ops._tiled_launch(kind, x, w, b, r, Cout, part, (mr, gw, gb, 32, silu) if gn else None)
            if stats:
                out["part"] = part
            if kind == "patch" and not stats and gn:      # gd_nn_conv3x3_gn_forward itself (_tiled_launch calls the _stats entry)
                y2 = torch.empty_like(out["y"])
                st = torch.cuda.current_stream().cuda_stream
                ret = L.gd_nn_conv3x3_gn_forward(st, x.data_ptr(), mr.data_ptr(), gw.data_ptr(), gb.data_ptr(), 32, silu,
                                                 w.data_ptr(), b.data_ptr(), 0, None, y2.data_ptr(), N, H, W, Cin, Cout)
                assert ret >= 0, L.gd_nn_conv_last_error().decode()
                out["y_gn_forward"] = y2
        torch.cuda.synchronize()
        saved = {}
        for k, v in out.items():
            v = v.cpu()
            assert bool(torch.isfinite(v.float()).all()), (kind, k)
            bits = v.view(torch.int16 if v.dtype == torch.bfloat16 else torch.int32)     # (a NaN would not equal itself)
            saved[k] = bits if bits.numel() <= (1 << 22) else hashlib.sha256(bits.numpy().tobytes()).hexdigest()
        torch.save(saved, os.path.join(out_dir, f"case{i:02d}.pt"))
        del x, w, r, out, part
        torch.cuda.empty_cache()


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3])
    lib_a, lib_b = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as tmp:
        dirs = []
        for tag, lib in (("a", lib_a), ("b", lib_b)):
            d = os.path.join(tmp, tag)
            os.makedirs(d)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(lib), d])
            dirs.append(d)
        bad = 0
        for i, case in enumerate(CASES):
            a = torch.load(os.path.join(dirs[0], f"case{i:02d}.pt"))
            b = torch.load(os.path.join(dirs[1], f"case{i:02d}.pt"))
            assert a.keys() == b.keys()
            for k in a:
                eq = a[k] == b[k] if isinstance(a[k], str) else torch.equal(a[k], b[k])
                bad += not eq
                print(f"{str(case):52s} {k:13s} {'bit-equal' if eq else 'DIFFERENT'} "
                      f"({'sha256' if isinstance(a[k], str) else str(a[k].numel()) + ' values'})", flush=True)
        assert bad == 0, f"{bad} outputs differ between {lib_a} and {lib_b}"
        print(f"all {len(CASES)} cases bit-equal: {lib_a} vs {lib_b}")


if __name__ == "__main__":
    main()
