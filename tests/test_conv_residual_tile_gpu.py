"""The convolution epilogues that fetch their residual tile by LDS-DMA (csrc/nn_conv3x3.hip, res_tile_*).

Covered kernels (KINDS): the wide-tile kernel (csrc/nn_conv_wide.h) and the Winograd kernel (csrc/nn_conv_wino.h), each plain
and with the GroupNorm loader, and the patch-staged GroupNorm kernel conv3x3_gn_patch_kernel (every GroupNorm launch of the
"patch" entry; its plain launches run the persistent streaming kernel, which keeps the per-lane loads).  Every launch goes to the kernel's own C entry with a
residual, not through ``nn_ops._conv_route``.  Full pixel tiles (16 x 32 wide, 16 x 16 patch and Winograd) whose channel slab lies below
Cout take the new path, every other tile of the same launch the per-lane loads, so the shapes put both into one output:

  * H x W = 16 x 16 (wide: no full tile), 16 x 32, 20 x 40 and 17 x 33 (full tiles and ragged ones in both directions);
  * one, two and three K chunks -- the idle patch stage that receives the first round alternates with the parity, and with
    one chunk the last chunk is the first: Cin = 32, 64, 96 (wide and Winograd, 32-channel chunks), 64, 128, 192 (patch, 64-channel chunks);
  * Cout = 128 and 320 (the third channel block ends beyond Cout and stays on the old path); patch also 256, its
    256-channel slab with four rounds per wave (128 and 320 run the 128-channel slab, two rounds);
  * N = 1 and 3, with and without bias, with and without the epilogue statistics, GroupNorm loader on and off.

Three kinds of assertion:
  1. zero weights, zero bias, random bf16 residual: the output IS the residual, bit for bit, and the guard bands around the
     output buffer keep their bytes -- this pins the addressing of the new path;
  2. small-integer operands (tests/exact_reference.py): every sum is exact, the output equals the float64 reference bit
     for bit, residual included;
  3. random operands against fp32 PyTorch at the bar of these kernels (2e-2 of scale, cos >= 0.9995).
With statistics, the rows summed in float64 equal the sums over the stored output to 1e-5.
"""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import exact_reference as X
from tests.exact_reference import int_operands

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
EPS = 1e-6
GUARD = 4096            # bf16 elements on either side of the output (a multiple of 8: the output stays 16-byte aligned)
GUARD_BITS = 0x7fc1     # a NaN pattern no kernel produces

KINDS = ["wide", "patch", "wino"]
LOADERS = {"wide": (0, 1), "patch": (1,), "wino": (0, 1)}        # GroupNorm loader off / on
CINS = {"wide": (32, 64, 96), "patch": (64, 128, 192), "wino": (32, 64, 96)}
COUTS = {"wide": (128, 320), "patch": (128, 256, 320), "wino": (128, 320)}
SHAPES = [(16, 16), (16, 32), (20, 40), (17, 33)]
CASES = [(k, H, W, Cin, Cout, N) for k in KINDS for (H, W) in SHAPES for Cin in CINS[k] for Cout in COUTS[k] for N in (1, 3)]
GROUPS = 8


def _rng(*case):
    return np.random.default_rng(zlib.crc32(repr(case).encode()))


def _variants(kind):
    return [(bias, stats, gn) for bias in (0, 1) for stats in (0, 1) for gn in LOADERS[kind]]


def _bf(t):
    t = t.to(torch.bfloat16).to(DEV)
    return t.contiguous(memory_format=CL) if t.dim() == 4 else t.contiguous()


def _launch(kind, x, w, bias, r, Cout, stats, gn):
    """The kernel's C entry on an output that lies between two guard bands.  Returns (y, statistics rows or None)."""
    from garmentdreamer_amd import nn_ops
    L = nn_ops.lib()
    N, Cin, H, W = x.shape
    assert kind == "patch" or bool(getattr(L, f"gd_nn_conv3x3_{kind}_supported")(N, H, W, Cin, Cout))
    n = N * H * W * Cout
    buf = torch.full((n + 2 * GUARD,), GUARD_BITS, dtype=torch.int16, device=DEV)
    y = buf[GUARD:GUARD + n].view(torch.bfloat16)
    rows = ((H + 15) // 16) * ((W + 15) // 16) * 8
    part = torch.full((N * (Cout // 4) * rows * 2,), float("nan"), dtype=torch.float32, device=DEV) if stats else None
    plain, gname = nn_ops._TILED_ENTRY[kind]
    name, head = (plain, ()) if gn is None else (gname, (gn[0].data_ptr(), gn[1].data_ptr(), gn[2].data_ptr(), gn[3], gn[4]))
    bias, stride = nn_ops._bias_and_stride(bias)
    ret = getattr(L, name)(torch.cuda.current_stream().cuda_stream, x.data_ptr(), *head, (w if kind == "patch" else nn_ops._packed(w, kind)).data_ptr(),
                           None if bias is None else bias.data_ptr(), stride, r.data_ptr(), y.data_ptr(), N, H, W, Cin, Cout,
                           None if part is None else part.data_ptr())
    assert ret >= 0, L.gd_nn_conv_last_error().decode()
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == GUARD_BITS).all()) and bool((buf[GUARD + n:] == GUARD_BITS).all()), "guard band overwritten"
    y = y.view(N, H, W, Cout).permute(0, 3, 1, 2)        # logical NCHW over the NHWC bytes
    if stats:
        assert bool(torch.isfinite(part).all()), "a statistics row was never written"
        got = part.view(N, Cout // 4, rows, 2).double().sum(2)
        yq = y.permute(0, 2, 3, 1).double().reshape(N, H * W, Cout // 4, 4)
        want = torch.stack([yq.sum((1, 3)), (yq * yq).sum((1, 3))], -1)
        assert ((got - want).abs().max() / want.abs().max().clamp_min(1e-30)).item() < 1e-5, "statistics rows"
    return y


def _mean_rstd(x, groups):
    xg = x.float().reshape(x.shape[0], groups, -1)
    return torch.stack([xg.mean(-1), (xg.var(-1, unbiased=False) + EPS).rsqrt()], -1).reshape(-1).contiguous()


@pytest.mark.parametrize("case", CASES, ids=str)
def test_zero_weights_return_the_residual_bit_for_bit(case):
    kind, H, W, Cin, Cout, N = case
    g = torch.Generator(DEV).manual_seed(zlib.crc32(repr(case).encode()))
    x = _bf(torch.randn(N, Cin, H, W, device=DEV, generator=g))
    w = _bf(torch.zeros(Cout, Cin, 3, 3))
    r = torch.randn(N, Cout, H, W, device=DEV, generator=g) * 3
    r = _bf(torch.where(r == 0, torch.ones_like(r), r))      # no zeros: 0 + -0 is +0, not the residual's bits
    gn_on = (_mean_rstd(x, GROUPS), _bf(torch.randn(Cin, device=DEV, generator=g) + 1), _bf(torch.randn(Cin, device=DEV, generator=g)),
             GROUPS, 1)
    for bias, stats, gn in _variants(kind):
        y = _launch(kind, x, w, _bf(torch.zeros(Cout)) if bias else None, r, Cout, stats, gn_on if gn else None)
        same = y.view(torch.int16) == r.view(torch.int16)
        assert bool(same.all()), X.mismatch_report(y.double().cpu(), r.double().cpu(), f"{case} bias {bias} stats {stats} gn {gn}")


@pytest.mark.parametrize("case", CASES, ids=str)
def test_small_integer_operands_are_exact_with_the_residual(case):
    """Operands as in tests/test_nn_exact_gpu.py: +-1 at the density of exact_reference.int_operands (plain), an exact affine
    GroupNorm map with +-1 weights thinned by the map's mean square (GroupNorm); bias and residual dense in [-4, 4]."""
    kind, H, W, Cin, Cout, N = case
    rng = _rng("exact", *case)
    K = 9 * Cin
    dense = lambda shape: int_operands(shape, None, rng, -4, 4)
    b, r = dense((N, Cout)), dense((N, Cout, H, W))
    # plain
    xp, wp = int_operands((N, Cin, H, W), K, rng), int_operands((Cout, Cin, 3, 3), K, rng)
    # GroupNorm as an exact affine map (test_nn_exact_gpu.gn_conv_ops)
    xg = 2.0 * int_operands((N, Cin, H, W), 1, rng)
    rstd = np.array([0.5, 1.0, 2.0])[rng.integers(0, 3, size=(N, GROUPS))]
    mean = rng.integers(-2, 3, size=(N, GROUPS)).astype(np.float64)
    mean = torch.from_numpy(np.where(rstd == 0.5, mean - np.mod(mean, 2), mean))
    rstd = torch.from_numpy(rstd)
    gamma = torch.from_numpy(np.array([-2.0, -1.0, 1.0, 2.0])[rng.integers(0, 4, size=(Cin,))])
    beta = torch.from_numpy(2.0 * rng.integers(-2, 3, size=(Cin,)).astype(np.float64))
    t, _, _ = X.gn_affine_ref(xg, mean, rstd, gamma, beta)
    wg = int_operands((Cout, Cin, 3, 3), K, rng, p=min(2.0 / 3.0, X.SUM_VARIANCE / (K * float((t * t).mean()))))
    conv = {gn: X.conv3x3_ref(t, wg) if gn else X.conv3x3_ref(xp, wp) for gn in LOADERS[kind]}   # float64, once per loader
    mr = torch.stack([mean, rstd], -1).reshape(-1).float().to(DEV).contiguous()
    for bias, stats, gn in _variants(kind):
        ref = conv[gn] + r + (b[:, :, None, None] if bias else 0.0)
        y = _launch(kind, _bf(xg if gn else xp), _bf(wg if gn else wp), _bf(b) if bias else None, _bf(r), Cout, stats,
                    (mr, _bf(gamma), _bf(beta), GROUPS, 0) if gn else None)
        X.assert_exact(y, ref, f"{case} bias {bias} stats {stats} gn {gn}")


@pytest.mark.parametrize("case", CASES, ids=str)
def test_random_operands_match_fp32_pytorch(case):
    kind, H, W, Cin, Cout, N = case
    g = torch.Generator(DEV).manual_seed(zlib.crc32(repr(("random",) + case).encode()))
    x = _bf(torch.randn(N, Cin, H, W, device=DEV, generator=g) * 1.5 + 0.3)
    w = _bf(torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (3 * Cin ** 0.5))
    b = _bf(torch.randn(Cout, device=DEV, generator=g))
    r = _bf(torch.randn(N, Cout, H, W, device=DEV, generator=g))
    gw, gb = _bf(torch.randn(Cin, device=DEV, generator=g) * 0.5 + 1), _bf(torch.randn(Cin, device=DEV, generator=g) * 0.5)
    act = {0: x.float(), 1: F.silu(F.group_norm(x.float(), GROUPS, gw.float(), gb.float(), EPS))}
    conv = {gn: F.conv2d(act[gn], w.float(), None, padding=1) for gn in LOADERS[kind]}
    for bias, stats, gn in _variants(kind):
        ref = conv[gn] + r.float() + (b.float()[None, :, None, None] if bias else 0.0)
        y = _launch(kind, x, w, b if bias else None, r, Cout, stats, (_mean_rstd(x, GROUPS), gw, gb, GROUPS, 1) if gn else None)
        err = ((y.float() - ref).abs().max() / ref.abs().max()).item()
        cos = F.cosine_similarity(y.float().flatten(), ref.flatten(), dim=0).item()
        assert err < 2e-2 and cos > 0.9995, (case, bias, stats, gn, err, cos)
