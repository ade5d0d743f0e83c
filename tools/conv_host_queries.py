#!/usr/bin/env python
"""Table of the convolution library's pure host decisions -- scratch sizes, statistics rows, which shapes the Winograd / wide /
first-conv kernels accept -- one line per shape and route scale.  The queries launch nothing and need no device, so two
builds can be compared anywhere:

    python tools/conv_host_queries.py --lib A/libgd_nn.so > a.txt; python tools/conv_host_queries.py --lib B/libgd_nn.so > b.txt

Identical output = the host layer of the two builds routes and sizes identically on these shapes."""
import argparse
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def step_shapes():
    """(N, Cin, Cout, H) of _STEP_CONV_SHAPES in tests/test_nn_gpu.py (read as text: the test module wants a device)."""
    src = open(os.path.join(ROOT, "tests", "test_nn_gpu.py")).read()
    body = src[src.index("_STEP_CONV_SHAPES = ["):]
    body = body[:body.index("\n\n")]
    return [tuple(int(v) for v in m) for m in re.findall(r"\((\d+), (\d+), (\d+), (\d+)\)", body)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=os.path.join(ROOT, "garmentdreamer_amd", "libgd_nn.so"))
    L = C.CDLL(ap.parse_args().lib)
    sized = ["gd_nn_conv3x3_ws_bytes", "gd_nn_conv3x3_stat_rows", "gd_nn_conv3x3_s2_ws_bytes", "gd_nn_conv3x3_first_stat_rows"] + \
            [f"gd_nn_conv3x3_{k}_weights_bytes" for k in ("wino", "wide")]
    for name in sized:
        getattr(L, name).restype = C.c_size_t
    shapes = sorted({(n, ci, co, h, h) for _, ci, co, h in step_shapes() for n in (1, 2, 8, 16)})
    shapes += [(2, 64, 64, 17, 23), (2, 128, 64, 21, 19), (1, 64, 128, 9, 13)]        # the odd maps of the conv tests
    shapes += [(n, 1280, 1280, h, h) for h in (8, 16) for n in (1, 2, 8, 16)]         # small maps
    for scale in (1, 2, 8):
        assert L.gd_nn_conv_set_route_scale(scale) == 0
        for N, Cin, Cout, H, W in shapes:
            row = [L.gd_nn_conv3x3_ws_bytes(N, H, W, Cin, Cout),
                   L.gd_nn_conv3x3_stat_rows(N, H, W, Cout, 0), L.gd_nn_conv3x3_stat_rows(N, H, W, Cout, 1)]
            row += [L.gd_nn_conv3x3_s2_ws_bytes(N, H, W, Cin, Cout, pad, dgrad) for pad in (0, 1) for dgrad in (0, 1)]
            for k in ("wino", "wide"):
                row += [getattr(L, f"gd_nn_conv3x3_{k}_supported")(N, H, W, Cin, Cout),
                        getattr(L, f"gd_nn_conv3x3_{k}_weights_bytes")(Cout, Cin)]
            print(f"scale={scale} N={N} Cin={Cin} Cout={Cout} H={H} W={W}: ws={row[0]} stat_rows={row[1]},{row[2]} "
                  f"s2_ws={row[3]},{row[4]},{row[5]},{row[6]} wino={row[7]},{row[8]} wide={row[9]},{row[10]}")
        for N, H in sorted({(n, h) for n, _, _, h, _ in shapes}):       # the first convolution: 3 -> 128 (and 4 -> 320, refused)
            print(f"scale={scale} N={N} H={H} first: stat_rows={L.gd_nn_conv3x3_first_stat_rows(N, H, H, 3, 128)},"
                  f"{L.gd_nn_conv3x3_first_stat_rows(N, H, H, 4, 320)} "
                  f"dgrad={L.gd_nn_conv3x3_first_dgrad_supported(N, H, H, 3, 128)},{L.gd_nn_conv3x3_first_dgrad_supported(N, H, H, 4, 128)}")
    L.gd_nn_conv_set_route_scale(1)


if __name__ == "__main__":
    main()
