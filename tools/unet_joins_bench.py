#!/usr/bin/env python
"""The UNet's joins on the 8-view step's shapes (16 latents): own kernels (nn_ops.add_join / concat_join) vs aten add / cat,
and own kernel with partial sums + finish vs aten + the GroupNorm statistics pass where the consumer is a two-pass
GroupNorm of whole quads.  Device time per call from a hipGraph of 20 calls on a ring of tensors.
    python tools/unet_joins_bench.py [N]"""
import sys
import torch
import torch.nn as nn
sys.path.insert(0, ".")
import tools.ablib  # noqa: F401,E402
from garmentdreamer_amd import nn_ops  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16
ADDS = [(64, 320), (32, 640), (16, 1280), (8, 1280)]                 # the residual add that ends a Transformer2DModel
CATS = [(8, 1280, 1280, N), (16, 1280, 1280, N), (16, 1280, 640, N), (32, 1280, 640, N), (32, 640, 640, N), (32, 640, 320, N),
        (64, 640, 320, N), (64, 320, 320, N), (64, 320, 320, N // 2)]  # _UpBlock's skip joins; the last reads the shared conv_in output
RING = 4


def graph_time(fn, reps=20):
    fn(); fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (5 * reps)


def nhwc(n, c, hw):
    return torch.randn(n, c, hw, hw, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def stats_pass(x, groups=32, eps=1e-5):
    n, c, h, w = x.shape
    mr = torch.empty(n * groups * 2, dtype=torch.float32, device=x.device)
    nn_ops._check(nn_ops.lib().gd_nn_groupnorm_stats(torch.cuda.current_stream().cuda_stream, x.data_ptr(), n, h * w, c, groups,
                                                     eps, nn_ops._gn_workspace(x, n, groups).data_ptr(), mr.data_ptr()),
                  "gd_nn_groupnorm_stats")
    return mr


def one(label, concat, hw, c0, c1, nb):
    a = [nhwc(N, c0, hw) for _ in range(RING)]
    b = [nhwc(nb, c1 if concat else c0, hw) for _ in range(RING)]
    full = [t if nb == N else t.repeat(N // nb, 1, 1, 1).contiguous(memory_format=torch.channels_last) for t in b]
    cc = c0 + c1 if concat else c0
    norm = nn.GroupNorm(32, cc).to("cuda", torch.bfloat16)
    k = [0]

    def nxt():
        k[0] = (k[0] + 1) % RING
        return k[0]
    own = lambda: nn_ops._join(a[nxt()], b[k[0]], concat, None)                                   # noqa: E731
    aten = (lambda: torch.cat([a[nxt()], full[k[0]]], dim=1)) if concat else (lambda: a[nxt()] + full[k[0]])   # noqa: E731
    with torch.no_grad():
        t_own, t_aten = graph_time(own), graph_time(aten)
        line = f"{label:30s} own {t_own:6.1f} us   aten {t_aten:6.1f} us   x{t_aten / t_own:.2f}"
        two_pass = not nn_ops.lib().gd_nn_groupnorm_silu_fused_supported(N, hw * hw, cc, 32)
        if two_pass and (cc // 32) % 4 == 0:
            t_own_s = graph_time(lambda: nn_ops._join(a[nxt()], b[k[0]], concat, norm, stats=True))
            t_aten_s = graph_time(lambda: stats_pass(aten()))
            line += f"   | with the GroupNorm statistics: own + finish {t_own_s:6.1f} us   aten + statistics pass {t_aten_s:6.1f} us"
        elif two_pass:
            line += f"   | two-pass GroupNorm of {cc // 32} channels per group: keeps its statistics pass"
    print(line, flush=True)


print(f"N = {N} latents")
for hw, c in ADDS:
    one(f"add    {hw}x{hw} {c}", False, hw, c, 0, N)
for hw, c0, c1, nb in CATS:
    one(f"concat {hw}x{hw} {c0}+{c1}" + (f" (b: {nb} images)" if nb != N else ""), True, hw, c0, c1, nb)
