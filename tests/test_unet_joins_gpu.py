"""The UNet's join kernels (nn_ops.add_join / concat_join -> gd_nn_add_gn_partials / gd_nn_concat_gn_partials): the
result is bit-equal to the torch op it replaces, and the GroupNorm statistics finished from the partial sums the join
leaves are as accurate as those of the statistics kernel they replace (gd_nn_groupnorm_stats), against an fp64 reference
computed from the bf16 result.

Bound: the error of gd_nn_groupnorm_stats on the same tensor is measured in the test, and the join's may be twice that.
Every case runs on a standard-normal input and on one with a large common offset (mean 50, std 0.1), where the variance
is the small difference of two large sums.

GroupNorm(32) wherever its groups are whole 4-channel quads (what gd_nn_groupnorm_finish_partials adds up: 1280 + 640 ->
60 per group, 320 + 320 -> 20).  320 and 640 + 320 channels give 10 and 30 per group: those layers keep their statistics
kernel in the network (asserted below), and the partial sums of the shape are checked with 16 groups (20 and 60 per group,
the 640 | 320 seam still inside a group).

Measured on MI355X (max over the cases; join / statistics kernel): |mean - ref| 1.8e-9 / 1.9e-9 on the normal inputs and
3.8e-6 / 3.8e-6 at mean 50 (the rounding of the fp32 result); rstd relative error 9.1e-8 / 8.8e-8 and 7.2e-8 / 7.2e-8
(PERF.md has the per-case table).
"""
import pytest
import torch
import torch.nn as nn

from garmentdreamer_amd import nn_ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

#        name              N  Nb   H   W   C0    C1  groups
CASES = [("add",           4,  4, 12, 20, 320,    0, 16),     # pixel count no multiple of the row block
         ("add_shared",    4,  2, 12, 20, 320,    0, 16),     # b holds 2 images: read at n % 2
         ("cat_1280_640",  2,  2,  8,  8, 1280, 640, 32),     # groups of 60 straddle the seam
         ("cat_640_320",   2,  2,  8,  8, 640,  320, 16),     # second straddling seam
         ("cat_shared",    4,  2, 16, 16, 320,  320, 32)]     # shared source
DISTS = [("normal", 0.0, 1.0), ("offset", 50.0, 0.1)]


def _nhwc(n, c, h, w, mean, std, seed):
    g = torch.Generator(DEV).manual_seed(seed)
    x = torch.randn(n, h, w, c, device=DEV, generator=g) * std + mean
    return x.to(torch.bfloat16).permute(0, 3, 1, 2)      # channels_last [n, c, h, w]


def _reference_stats(out, groups, eps):
    n, c, h, w = out.shape
    x = out.double().reshape(n, groups, c // groups, h * w)
    mean = x.mean(dim=(2, 3))
    var = x.var(dim=(2, 3), unbiased=False)
    return mean, (var + eps).rsqrt()


def _errors(mr, mean, rstd):
    mr = mr.view(mean.shape[0], mean.shape[1], 2).double()
    return (mr[..., 0] - mean).abs().max().item(), ((mr[..., 1] - rstd).abs() / rstd).max().item()


def _kernel_stats(out, groups, eps):
    """mean / rstd of today's statistics kernel on the same tensor."""
    N, Cc, H, W = out.shape
    mr = torch.empty(N * groups * 2, dtype=torch.float32, device=out.device)
    ws = nn_ops._gn_workspace(out, N, groups)
    nn_ops._check(nn_ops.lib().gd_nn_groupnorm_stats(torch.cuda.current_stream().cuda_stream, out.data_ptr(), N, H * W, Cc,
                                                     groups, float(eps), ws.data_ptr(), mr.data_ptr()), "gd_nn_groupnorm_stats")
    return mr


@pytest.mark.parametrize("dist", DISTS, ids=[d[0] for d in DISTS])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_join_is_bit_equal_to_torch_and_leaves_the_groupnorm_statistics(case, dist):
    name, N, Nb, H, W, C0, C1, groups = case
    _, mean, std = dist
    concat = C1 > 0
    a = _nhwc(N, C0, H, W, mean, std, 1)
    b = _nhwc(Nb, C1 if concat else C0, H, W, mean, std, 2)
    norm = nn.GroupNorm(groups, C0 + C1, eps=1e-5).to(DEV, torch.bfloat16)
    b_full = b.repeat(N // Nb, 1, 1, 1)
    with torch.no_grad():
        want = torch.cat([a, b_full], dim=1) if concat else a + b_full
        assert nn_ops.join_supported(a, b)
        # (stats=True: these small maps would take the one-launch GroupNorm, for which the routing asks for no partial sums)
        got = nn_ops._join(a, b, concat, norm, stats=True)
        plain = nn_ops._join(a, b, concat, None)                                   # no consumer named: no statistics
        routed = (nn_ops.concat_join if concat else nn_ops.add_join)(a, b, norm)   # what the network calls
        assert torch.equal(routed.view(torch.int16), want.view(torch.int16)), name
    assert got.shape == want.shape and got.dtype == torch.bfloat16
    assert got.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), name
    assert torch.equal(plain.view(torch.int16), want.view(torch.int16)), name
    assert nn_ops.gn_stats_of(plain, groups, norm.eps) is None
    mr = nn_ops.gn_stats_of(got, groups, norm.eps)
    assert mr is not None, "the join left no statistics for a GroupNorm of whole quads on the two-pass path"
    ref_mean, ref_rstd = _reference_stats(got, groups, norm.eps)
    e_mean, e_rstd = _errors(mr, ref_mean, ref_rstd)
    k_mean, k_rstd = _errors(_kernel_stats(got, groups, norm.eps), ref_mean, ref_rstd)
    print(f"{name}/{dist[0]}: join |dmean| {e_mean:.3e} rel drstd {e_rstd:.3e}; statistics kernel {k_mean:.3e} {k_rstd:.3e}")
    assert e_mean <= 2 * k_mean, (e_mean, k_mean)
    assert e_rstd <= 2 * k_rstd, (e_rstd, k_rstd)
    # the statistics are reproducible from run to run (plain stores, fixed order) ...
    with torch.no_grad():
        again = nn_ops._join(a, b, concat, norm, stats=True)
    assert torch.equal(nn_ops.gn_stats_of(again, groups, norm.eps), mr)
    # ... and the GroupNorm that takes them gives what its own statistics pass gives, to the rounding of the output
    with torch.no_grad():
        y_mr = nn_ops._GroupNormSiLU.apply(got, norm.weight, norm.bias, groups, norm.eps, True, mr)     # apply pass only
        y_own = nn_ops._GroupNormSiLU.apply(got, norm.weight, norm.bias, groups, norm.eps, True)
    # z = (x - mean) rstd (unit gain): the two statistics move z by |z| (relative rstd errors) + rstd (mean errors), SiLU's
    # slope is at most 1.1, and the bf16 result may then round the other way (one ulp at the largest value)
    scale = y_own.float().abs().max().item()
    tol = 2 ** -7 * scale + 1.1 * (scale * (e_rstd + k_rstd) + ref_rstd.max().item() * (e_mean + k_mean))
    assert (y_mr.float() - y_own.float()).abs().max().item() <= tol


def test_groups_that_are_not_whole_quads_keep_the_statistics_kernel():
    """320 channels in 32 groups are 10 per group: no partial sums are written even when asked for, nothing rides on the
    result, and the GroupNorm runs its own statistics pass."""
    a, b = _nhwc(2, 320, 8, 8, 0.0, 1.0, 3), _nhwc(2, 320, 8, 8, 0.0, 1.0, 4)
    norm = nn.GroupNorm(32, 320).to(DEV, torch.bfloat16)
    with torch.no_grad():
        got = nn_ops._join(a, b, False, norm, stats=True)
        assert nn_ops.gn_stats_of(got, 32, norm.eps) is None
        assert torch.equal(got, a + b)


def test_a_written_tensor_drops_its_statistics_and_entry_points_refuse_bad_arguments():
    a, b = _nhwc(2, 640, 8, 8, 0.0, 1.0, 5), _nhwc(2, 640, 8, 8, 0.0, 1.0, 6)
    norm = nn.GroupNorm(32, 1280).to(DEV, torch.bfloat16)
    with torch.no_grad():
        # the network's routing asks for no statistics unless switched on (GD_NN_JOIN_STATS), and never where the one-launch
        # GroupNorm runs (1280 channels on an 8x8 map): it has no statistics pass to save
        assert nn_ops.gn_stats_of(nn_ops.concat_join(a, b, norm), 32, norm.eps) is None
        assert not nn_ops._join_wants_stats(2, 64, 1280, norm)
        other = nn.GroupNorm(32, 1280, eps=1e-6).to(DEV, torch.bfloat16)
        big = nn_ops._join(_nhwc(1, 640, 64, 64, 0.0, 1.0, 7), _nhwc(1, 640, 64, 64, 0.0, 1.0, 8), True, other, stats=True)
        assert nn_ops.gn_stats_of(big, 32, 1e-6) is not None and nn_ops.gn_stats_of(big, 32, 1e-5) is None
        big.add_(1)
        assert nn_ops.gn_stats_of(big, 32, 1e-6) is None
    L = nn_ops.lib()
    s = torch.cuda.current_stream().cuda_stream
    o = torch.empty(2, 1280, 8, 8, device=DEV, dtype=torch.bfloat16)
    assert L.gd_nn_add_gn_partials(s, a.data_ptr(), b.data_ptr(), o.data_ptr(), None, 2, 2, 64, 644) < 0        # C % 8
    assert L.gd_nn_add_gn_partials(s, a.data_ptr(), b.data_ptr(), o.data_ptr(), None, 3, 2, 64, 640) < 0        # 3 % 2
    assert L.gd_nn_concat_gn_partials(s, a.data_ptr(), b.data_ptr(), o.data_ptr(), None, 2, 2, 64, 2048, 1024) < 0
    assert L.gd_nn_concat_gn_partials(s, None, b.data_ptr(), o.data_ptr(), None, 2, 2, 64, 640, 640) < 0
    assert L.gd_nn_join_stat_rows(2, 64, 644) == 0
