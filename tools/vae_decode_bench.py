"""Time the SD-2.1 VAE decode (sd21.AutoencoderKL.decode_to_image) on MI355X: the own path (fused stem / head kernels,
channels_last bf16 weights) against the same module on the library path (the same weights stored NCHW-contiguous, so every
convolution goes to MIOpen, with the stem / head as PyTorch ops), at N = 1, 4 and 8 on 64^2 latents; and the head
kernel alone (gd_nn_vae_decoder_head, statistics supplied) in GB/s against the 6.3 TB/s streaming roof.

    python tools/vae_decode_bench.py [--reps 10] [--out FILE]
"""
from __future__ import annotations

import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import garmentdreamer_amd  # noqa: E402,F401
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda:0"
ROOF_GBS = 6300.0


def _time(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def library_decode(m, lat):
    """decode_to_image's expression with every layer on PyTorch's ops (NCHW weights: MIOpen convolutions)."""
    d = m.decoder
    with torch.no_grad():
        z = (lat * (1.0 / m.config.scaling_factor)).to(torch.bfloat16)
        x = d.body(d.conv_in(m.post_quant_conv(z)))
        r = d.conv_out(F.silu(d.conv_norm_out(x)))
        return (r.float() * 0.5 + 0.5).clamp(0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from garmentdreamer_amd import nn_ops
    from garmentdreamer_amd.guidance import sd21
    with torch.device(DEV):
        vae = sd21.init_random_(sd21.AutoencoderKLDecoder(), 2)
    own = vae.to(torch.bfloat16).to(memory_format=torch.channels_last).eval().requires_grad_(False)
    lib = copy.deepcopy(own).to(memory_format=torch.contiguous_format)
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; median (min) of {args.reps} timed runs"]
    lines.append("kernels alone (statistics of the head supplied): bytes = input read once + output written once")
    lines.append(f"{'kernel':<28} {'N':>3} {'us':>9} {'GB/s':>8} {'of roof':>8}")
    d = own.decoder
    n = d.conv_norm_out
    for N in (1, 4, 8):
        x = (torch.randn(N, 128, 512, 512, device=DEV) * 1.3).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        xf = x.float().reshape(N, 32, -1)
        mr = torch.stack([xf.mean(-1), torch.rsqrt(xf.var(-1, unbiased=False) + 1e-6)], -1).reshape(-1).contiguous()
        del xf
        for mode, out_bytes in (("image", 12), ("raw", 6)):
            t, _ = _time(lambda: nn_ops.vae_decode_head(x, n.weight, n.bias, 32, 1e-6, d.conv_out.weight, d.conv_out.bias,
                                                        mode, mean_rstd=mr), args.reps * 3)
            gbs = (x.numel() * 2 + N * 512 * 512 * out_bytes) / (t * 1e-3) / 1e9
            lines.append(f"{'head (' + mode + ')':<28} {N:>3} {t * 1e3:>9.1f} {gbs:>8.0f} {gbs / ROOF_GBS:>7.0%}")
            print(lines[-1], flush=True)
        t, _ = _time(lambda: nn_ops.vae_decode_head(x, n.weight, n.bias, 32, 1e-6, d.conv_out.weight, d.conv_out.bias,
                                                    "image"), args.reps * 3)
        lines.append(f"{'GroupNorm stats + head':<28} {N:>3} {t * 1e3:>9.1f}")
        lat = torch.randn(N, 4, 64, 64, device=DEV)
        pq = own.post_quant_conv
        t, _ = _time(lambda: nn_ops.vae_decode_stem(lat, 1 / 0.18215, pq.weight, pq.bias, d.conv_in.weight, d.conv_in.bias),
                     args.reps * 3)
        gbs = (lat.numel() * 4 + N * 64 * 64 * 512 * 2) / (t * 1e-3) / 1e9
        lines.append(f"{'stem (fp32 latents)':<28} {N:>3} {t * 1e3:>9.1f} {gbs:>8.0f} {gbs / ROOF_GBS:>7.0%}")
        print(lines[-1], flush=True)
        del x
    lines.append("")
    lines.append("decode_to_image, 64x64 latents -> 512x512 fp32 images")
    lines.append(f"{'N':>3} {'own ms':>10} {'library ms':>12} {'speed-up':>9} {'own ms/img':>11} {'max|own-lib|':>13}")
    for N in (1, 4, 8):
        lat = torch.randn(N, 4, 64, 64, device=DEV, generator=torch.Generator(DEV).manual_seed(N)) * 0.7
        t_own, m_own = _time(lambda: own.decode_to_image(lat), args.reps)
        t_lib, m_lib = _time(lambda: library_decode(lib, lat), args.reps)
        diff = (own.decode_to_image(lat) - library_decode(lib, lat)).abs().max().item()
        lines.append(f"{N:>3} {t_own:>7.2f} ({m_own:.2f}) {t_lib:>8.2f} ({m_lib:.2f}) {t_lib / t_own:>8.2f}x {t_own / N:>11.2f} "
                     f"{diff:>13.3e}")
        print(lines[-1], flush=True)
    fallbacks = nn_ops.library_fallbacks(reset=True)
    lines.append(f"library fallbacks counted (all from the library-path module): {sum(fallbacks.values())}")

    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
