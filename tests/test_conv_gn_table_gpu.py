"""The GroupNorm-in-the-loader convolutions read scale / shift from a per-image LDS table (csrc/nn_device.h, gn_table_*).

Every case calls the C entry of ONE kernel through ``nn_ops._tiled_launch(kind, ..., gn=...)``, so no routing threshold
hides a kernel: "wide" (csrc/nn_conv_wide.h), "patch" (conv3x3_gn_patch_kernel) and "wino" (csrc/nn_conv_wino.h).  The
persistent streaming kernel has no GroupNorm entry (launch_patch sends every GroupNorm launch to conv3x3_gn_patch_kernel;
conv3x3_patch_stream_kernel<.., GN = true> is not instantiated), so there is nothing of it to call here.

What can go wrong with a table and is pinned here:
  * the channel -> group map when an 8-channel octet lies inside one group (Cin / G = 2, 4: several octets or several
    groups per octet) or spans two or three groups (Cin / G = 5, 10), in every K chunk;
  * a table of the WRONG image: batches of 3 and 5 images with strongly different statistics, more tiles than the chip has
    compute units, bit-equal to each image run alone and to the permuted batch;
  * the table next to the epilogue's use of LDS (transposition buffer, statistics) with a residual, SiLU on and off.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
EPS = 1e-6


def _supported(kind, N, H, W, Cin, Cout):
    from garmentdreamer_amd import nn_ops
    if kind == "patch":     # launch_patch: Cin % 64 == 0, Cout % 4 == 0 (it has no _supported entry of its own)
        return Cin % 64 == 0 and Cout % 4 == 0
    return bool(getattr(nn_ops.lib(), f"gd_nn_conv3x3_{kind}_supported")(N, H, W, Cin, Cout))


def _mean_rstd(x, groups):
    xg = x.float().reshape(x.shape[0], groups, -1)
    return torch.stack([xg.mean(-1), (xg.var(-1, unbiased=False) + EPS).rsqrt()], -1).reshape(-1).contiguous()


def _case(N, Cin, Cout, H, W, seed, res=False, per_image=False):
    """bf16 operands of one layer; per_image: image n scaled by n + 1 and shifted by n (statistics that differ strongly)."""
    g = torch.Generator(DEV).manual_seed(seed)
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g) * 1.5 + 0.3
    if per_image:
        n = torch.arange(N, device=DEV, dtype=torch.float32).view(N, 1, 1, 1)
        x = x * (n + 1) + n
    x = x.to(torch.bfloat16).contiguous(memory_format=CL)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (3 * Cin ** 0.5)).to(torch.bfloat16).contiguous(memory_format=CL)
    b = torch.randn(Cout, device=DEV, generator=g).to(torch.bfloat16)
    r = torch.randn(N, Cout, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=CL) if res else None
    gw = (torch.randn(Cin, device=DEV, generator=g) * 0.5 + 1).to(torch.bfloat16)
    gb = (torch.randn(Cin, device=DEV, generator=g) * 0.5).to(torch.bfloat16)
    return x, w, b, r, gw, gb


def _reference(x, w, b, r, gw, gb, groups, silu):
    a = F.group_norm(x.float(), groups, gw.float(), gb.float(), EPS)
    y = F.conv2d(F.silu(a) if silu else a, w.float(), b.float(), padding=1)
    return y + r.float() if r is not None else y


def _assert_close(y, ref):
    """The conv bar of tests/test_nn_gpu.py: 2e-2 of scale, cos > 0.9995."""
    err = ((y.float() - ref).abs().max() / ref.abs().max()).item()
    cos = F.cosine_similarity(y.float().flatten(), ref.flatten(), dim=0).item()
    print(f"err {err:.3e} of scale, cos {cos:.6f}")
    assert err < 2e-2 and cos > 0.9995, (err, cos)


# Cin / G = 2, 4 (octets inside groups), 5 and 10 (an octet spans two or three groups; 160 = five 32-channel chunks for
# the wide and Winograd kernels, 320 = five 64-channel chunks for the patch kernel).  20 x 40 pixels: ragged against the
# 16 x 16 and 16 x 32 tiles in both directions, two tile rows, N = 2 -> the second image's statistics row.
_OCTET_CASES = [("wide", 64), ("wide", 128), ("wide", 160), ("wide", 320), ("wino", 64), ("wino", 128), ("wino", 160),
                ("wino", 320), ("patch", 64), ("patch", 128), ("patch", 320)]


@pytest.mark.parametrize("kind,Cin", _OCTET_CASES)
def test_groups_against_channel_octets_match_fp32_reference(kind, Cin):
    from garmentdreamer_amd import nn_ops
    N, Cout, H, W, groups = 2, 64, 20, 40, 32
    assert _supported(kind, N, H, W, Cin, Cout)
    x, w, b, r, gw, gb = _case(N, Cin, Cout, H, W, seed=Cin * 3 + len(kind), per_image=True)
    with torch.no_grad():
        y = nn_ops._tiled_launch(kind, x, w, b, r, Cout, gn=(_mean_rstd(x, groups), gw, gb, groups, True))
        _assert_close(y, _reference(x, w, b, r, gw, gb, groups, True))


# More tiles than the 256 compute units (wide: 12 x 8 = 96 tiles of 16 x 32 per image -> 288 / 480; patch and Winograd:
# 10 x 10 = 100 tiles of 16 x 16 -> 300 / 500), so a compute unit works through tiles of several images one after the
# other and the XCD-contiguous tile order is in force for N = 3 on the wide tile (288 % 8 == 0) and off elsewhere.
_BATCH_CASES = [("wide", 3, 192, 256), ("wide", 5, 192, 256), ("patch", 3, 160, 160), ("patch", 5, 160, 160),
                ("wino", 3, 160, 160), ("wino", 5, 160, 160)]


@pytest.mark.parametrize("kind,N,H,W", _BATCH_CASES)
def test_each_image_of_a_batch_gets_its_own_table(kind, N, H, W):
    """Bit-exact: image n of the batch equals the same image run alone, and a permuted batch gives the permuted outputs
    (an output pixel's summation order does not depend on the batch)."""
    from garmentdreamer_amd import nn_ops
    Cin, Cout, groups = 64, 64, 32
    assert _supported(kind, N, H, W, Cin, Cout)
    x, w, b, _, gw, gb = _case(N, Cin, Cout, H, W, seed=N * 11 + H, per_image=True)
    mr = _mean_rstd(x, groups)
    assert (mr.view(N, groups, 2)[0, :, 1] / mr.view(N, groups, 2)[N - 1, :, 1]).min().item() > 2   # tables that differ
    with torch.no_grad():
        y = nn_ops._tiled_launch(kind, x, w, b, None, Cout, gn=(mr, gw, gb, groups, True))
        for n in range(N):
            xn = x[n:n + 1].contiguous(memory_format=CL)
            yn = nn_ops._tiled_launch(kind, xn, w, b, None, Cout,
                                      gn=(mr.view(N, -1)[n].contiguous(), gw, gb, groups, True))
            assert torch.equal(yn[0], y[n]), f"image {n} of the batch differs from the image run alone"
        perm = torch.tensor([(i + 1) % N for i in range(N)], device=DEV)       # no image keeps its place
        xp = x[perm].contiguous(memory_format=CL)
        yp = nn_ops._tiled_launch(kind, xp, w, b, None, Cout,
                                  gn=(mr.view(N, -1)[perm].reshape(-1).contiguous(), gw, gb, groups, True))
        assert torch.equal(yp, y[perm]), "permuting the images does not permute the outputs"


@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("kind", ["wide", "patch", "wino"])
def test_table_does_not_disturb_the_epilogue(kind, silu):
    """Residual and epilogue statistics on: the epilogue's transposition buffer lies in the stages below the table."""
    from garmentdreamer_amd import nn_ops
    N, Cin, Cout, H, W, groups = 2, 128, 136, 36, 40, 32
    assert _supported(kind, N, H, W, Cin, Cout)
    x, w, b, r, gw, gb = _case(N, Cin, Cout, H, W, seed=77 + silu, res=True, per_image=True)
    rows = ((H + 15) // 16) * ((W + 15) // 16) * 8
    part = torch.full((N * (Cout // 4) * rows * 2,), float("nan"), dtype=torch.float32, device=DEV)   # every row must be written
    with torch.no_grad():
        y = nn_ops._tiled_launch(kind, x, w, b, r, Cout, part, (_mean_rstd(x, groups), gw, gb, groups, silu))
        _assert_close(y, _reference(x, w, b, r, gw, gb, groups, bool(silu)))
    assert torch.isfinite(part).all()
    got = part.view(N, Cout // 4, rows, 2).double().sum(2)
    yq = y.permute(0, 2, 3, 1).float().double().reshape(N, H * W, Cout // 4, 4)
    want = torch.stack([yq.sum((1, 3)), (yq * yq).sum((1, 3))], -1)
    assert ((got - want).abs().max() / want.abs().max()).item() < 1e-5
