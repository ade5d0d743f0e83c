"""CPU side of the UNet joins and the shared guidance prefix: without a GPU the new arguments run the torch ops and give
the tensors of the old code, and the guidance hands ``shared_reps`` only to a UNet that takes it, only where it builds the
repeated batch itself."""
import torch
import torch.nn as nn

from garmentdreamer_amd import nn_ops
from garmentdreamer_amd.guidance import sd21
from garmentdreamer_amd.guidance.stable_diffusion_guidance import PromptEmbeddings, StableDiffusionGuidance


def test_joins_on_cpu_are_the_torch_ops():
    g = torch.Generator().manual_seed(0)
    a = torch.randn(4, 16, 5, 3, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    b = torch.randn(4, 16, 5, 3, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    half = b[:2]
    norm = nn.GroupNorm(4, 16)
    assert not nn_ops.join_supported(a, b)
    s = nn_ops.add_join(a, b, norm)
    assert torch.equal(s, a + b) and nn_ops.gn_stats_of(s, 4, norm.eps) is None
    assert torch.equal(nn_ops.add_join(a, half), a + torch.cat([half, half]))
    assert torch.equal(nn_ops.concat_join(a, b, nn.GroupNorm(4, 32)), torch.cat([a, b], dim=1))
    assert torch.equal(nn_ops.concat_join(a, half), torch.cat([a, torch.cat([half, half])], dim=1))
    x = torch.randn(2, 16, 4, 4, generator=g)
    want = torch.nn.functional.silu(torch.nn.functional.group_norm(x, 4, norm.weight, norm.bias, norm.eps))
    assert torch.equal(nn_ops.group_norm_silu(x, norm.weight, norm.bias, 4, norm.eps, True, mean_rstd=None), want)


def test_add_layer_norm_and_attention_take_a_shared_operand_on_cpu():
    g = torch.Generator().manual_seed(1)
    ln = nn.LayerNorm(16)
    x, r = torch.randn(2, 6, 16, generator=g), torch.randn(4, 6, 16, generator=g)
    s, y = nn_ops.add_layer_norm(x, r, ln)
    want = torch.cat([x, x]) + r
    assert torch.equal(s, want) and torch.equal(y, ln(want))
    att = sd21.Attention(16, 2, 8, cross_dim=12)
    h, ctx = torch.randn(2, 6, 16, generator=g), torch.randn(4, 5, 12, generator=g)
    assert torch.equal(att(h, ctx, reps=2), att(torch.cat([h, h]), ctx))
    blk = sd21.BasicTransformerBlock(16, 2, 8, 12)
    assert torch.equal(blk(h, ctx, reps=2), blk(torch.cat([h, h]), ctx))
    tr = sd21.Transformer2DModel(16, 2, 8, 12, groups=4)
    img = torch.randn(2, 16, 3, 2, generator=g)
    assert torch.equal(tr(img, ctx, reps=2), tr(torch.cat([img, img]), ctx))
    assert torch.equal(tr(img, ctx[:2], next_norm=nn.GroupNorm(4, 16)), tr(img, ctx[:2]))


def test_route_batch_shared_divides_the_announced_batch():
    assert nn_ops._ROUTE_BATCH is None
    with nn_ops.route_batch_shared(2):
        assert nn_ops._ROUTE_BATCH is None
    with nn_ops.route_batch(2, 8):
        with nn_ops.route_batch_shared(2):
            assert nn_ops._ROUTE_BATCH == (1, 4)
            with nn_ops.route_batch_shared(2):      # does not divide: left as it is
                assert nn_ops._ROUTE_BATCH == (1, 4)
        with nn_ops.route_batch_shared(1):
            assert nn_ops._ROUTE_BATCH == (2, 8)
        assert nn_ops._ROUTE_BATCH == (2, 8)
    assert nn_ops._ROUTE_BATCH is None


class _StubUNet(nn.Module):
    """Records what the guidance hands over; computes something that depends on the sample, the timestep and the context."""

    def __init__(self, shares: bool):
        super().__init__()
        self.supports_shared_reps = shares
        self.w = nn.Parameter(torch.ones(1))
        self.calls = []

    def forward(self, x, t, encoder_hidden_states, **kw):
        self.calls.append((tuple(x.shape), tuple(t.shape), tuple(encoder_hidden_states.shape), dict(kw)))
        r = kw.get("shared_reps", 1)
        x, t = torch.cat([x] * r), torch.cat([t] * r)
        return x * self.w + 1e-3 * t.view(-1, 1, 1, 1).to(x.dtype) + encoder_hidden_states.mean(dim=(1, 2)).view(-1, 1, 1, 1).to(x.dtype)


class _StubVAE(nn.Module):
    config = sd21._VAEConfig()

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(1))

    def encode(self, x):
        m = torch.nn.functional.avg_pool2d(x, 8)[:, :1].repeat(1, 8, 1, 1) * self.w
        return sd21._EncodeOutput(sd21.DiagonalGaussianDistribution(m))


def _guidance_call(shares: bool, **cfg):
    unet = _StubUNet(shares)
    gd = StableDiffusionGuidance({"half_precision_weights": False, "use_hip_graphs": False, **cfg}, device="cpu", unet=unet,
                                 vae=_StubVAE())
    gd.update_step(0, 0)
    g = torch.Generator().manual_seed(2)
    rgb = torch.rand(2, 64, 64, 3, generator=g)
    out = gd(rgb, PromptEmbeddings.random("cpu"), torch.tensor([10.0, 20.0]), torch.tensor([0.0, 100.0]), torch.ones(2) * 2,
             noise=torch.randn(2, 4, 64, 64, generator=g), timesteps=torch.tensor([100, 700]),
             vae_noise=torch.randn(2, 4, 64, 64, generator=g))
    return unet, out["loss_sds"]


def test_guidance_passes_shared_reps_only_where_it_builds_the_repeated_batch():
    for cfg in ({}, {"use_sjc": True, "var_red": True}):
        plain, loss_plain = _guidance_call(False, **cfg)
        shared, loss_shared = _guidance_call(True, **cfg)
        assert plain.calls == [((4, 4, 64, 64), (4,), (4, 77, 1024), {})]
        assert shared.calls == [((2, 4, 64, 64), (2,), (4, 77, 1024), {"shared_reps": 2})]
        assert torch.equal(loss_plain, loss_shared)
    # a direct forward_unet call (the caller brings its own batch) passes nothing
    unet = _StubUNet(True)
    gd = StableDiffusionGuidance({"half_precision_weights": False, "use_hip_graphs": False}, device="cpu", unet=unet, vae=_StubVAE())
    gd.forward_unet(torch.zeros(4, 4, 8, 8), torch.zeros(4), torch.zeros(4, 77, 1024))
    assert unet.calls[-1][3] == {}


def test_unet_on_cpu_runs_shared_reps_as_the_repeated_batch():
    torch.manual_seed(0)
    unet = sd21.init_random_(sd21.UNet2DConditionModel(block_out_channels=(32, 32, 64, 64), attention_head_dim=(1, 1, 2, 2),
                                                       cross_attention_dim=16)).eval()
    g = torch.Generator().manual_seed(3)
    x, t, ctx = torch.randn(1, 4, 8, 8, generator=g), torch.tensor([400.0]), torch.randn(2, 5, 16, generator=g)
    with torch.no_grad():
        assert torch.equal(unet(x, t, ctx, shared_reps=2), unet(torch.cat([x, x]), torch.cat([t, t]), ctx))
    try:
        unet(x, t, ctx[:1], shared_reps=2)
    except ValueError:
        pass
    else:
        raise AssertionError("a context batch that is not reps x samples must be refused")
