"""GPU numerics of the hand-written guidance kernels vs plain PyTorch fp32 references of the same op."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("N,C,H,W,silu", [(2, 128, 32, 32, True), (3, 320, 16, 16, True), (2, 1280, 8, 8, False),
                                          (1, 2560, 8, 8, True), (2, 960, 16, 16, True), (2, 512, 24, 24, False),
                                          (1, 1920, 5, 7, True)])
def test_groupnorm_silu_matches_fp32_reference(N, C, H, W, silu):
    from garmentdreamer_amd.nn_ops import group_norm_silu
    g = torch.Generator(DEV).manual_seed(C + H)
    x32 = (torch.randn(N, C, H, W, device=DEV, generator=g) * 1.7 + 0.4)
    w32 = torch.randn(C, device=DEV, generator=g) * 0.5 + 1.0
    b32 = torch.randn(C, device=DEV, generator=g) * 0.3
    x = x32.to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w, b = w32.to(torch.bfloat16), b32.to(torch.bfloat16)
    y = group_norm_silu(x, w, b, 32, 1e-5, silu)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    xr = x.detach().float().requires_grad_(True)
    yr = F.group_norm(xr, 32, w.float(), b.float(), 1e-5)
    yr = F.silu(yr) if silu else yr
    err = (y.float() - yr).abs().max().item()
    assert err <= 2e-2 * yr.abs().max().item() + 1e-2, err     # bf16 output rounding
    gy = torch.randn(N, C, H, W, device=DEV, generator=g).to(torch.bfloat16)
    y.backward(gy)
    yr.backward(gy.float())
    gerr = (x.grad.float() - xr.grad).abs().max().item()
    assert gerr <= 2e-2 * xr.grad.abs().max().item() + 1e-3, gerr
    cos = F.cosine_similarity(x.grad.float().flatten(), xr.grad.flatten(), dim=0).item()
    assert cos > 0.9995, cos


@pytest.mark.parametrize("N,C,H,W,silu", [(2, 320, 32, 32, True), (16, 1280, 32, 32, True), (2, 1280, 8, 8, False),
                                          (3, 2560, 16, 16, True), (2, 1920, 32, 32, True), (2, 960, 32, 32, True),
                                          (2, 640, 32, 32, False), (1, 1920, 5, 7, True), (2, 128, 2, 2, True),
                                          (4, 1280, 16, 16, True)])
def test_one_launch_groupnorm_matches_fp32_reference_and_the_two_pass_kernels(N, C, H, W, silu):
    """Inference GroupNorm(+SiLU) of the UNet's maps in ONE launch (gd_nn_groupnorm_silu_fused_forward: one workgroup
    per (image, group), slice in registers) against fp32 torch at the GroupNorm bar, and against the two-pass
    kernels it replaces: same coefficients up to the last bit of mean / rstd, so the bf16 outputs may differ by one
    rounding step on a few elements, never more."""
    from garmentdreamer_amd import nn_ops
    assert nn_ops.lib().gd_nn_groupnorm_silu_fused_supported(N, H * W, C, 32) == 1
    g = torch.Generator(DEV).manual_seed(C + H + N)
    x = (torch.randn(N, C, H, W, device=DEV, generator=g) * 1.7 + 0.4).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(C, device=DEV, generator=g) * 0.5 + 1.0).to(torch.bfloat16)
    b = (torch.randn(C, device=DEV, generator=g) * 0.3).to(torch.bfloat16)
    with torch.no_grad():
        y = nn_ops.group_norm_silu(x, w, b, 32, 1e-5, silu)                 # no grad: the one-launch form
        y2 = nn_ops._GroupNormSiLU.apply(x, w, b, 32, 1e-5, silu)           # statistics kernel + apply kernel
        y_again = nn_ops.group_norm_silu(x, w, b, 32, 1e-5, silu)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y, y_again)                                          # no atomics: reproducible
    yr = F.group_norm(x.float(), 32, w.float(), b.float(), 1e-5)
    yr = F.silu(yr) if silu else yr
    assert (y.float() - yr).abs().max().item() <= 2e-2 * yr.abs().max().item() + 1e-2
    d = (y.float() - y2.float()).abs()
    ulp = torch.maximum(y2.float().abs(), torch.full_like(d, 2.0 ** -8)) * 2.0 ** -7      # one bf16 step at |y|
    assert bool((d <= ulp).all()), float((d / ulp).max())
    assert float((d > 0).float().mean()) < 2e-2
    # a tensor that needs a gradient takes the same launch with the statistics kept (its backward pass: the test below)
    xg = x.clone().requires_grad_(True)
    yg = nn_ops.group_norm_silu(xg, w, b, 32, 1e-5, silu)
    assert yg.grad_fn is not None and torch.equal(yg.detach(), y)


def test_one_launch_groupnorm_refuses_slices_that_do_not_fit_the_registers():
    from garmentdreamer_amd import nn_ops
    L = nn_ops.lib()
    assert L.gd_nn_groupnorm_silu_fused_supported(2, 64 * 64, 640, 32) == 0        # 160 KB per (image, group)
    assert L.gd_nn_groupnorm_silu_fused_supported(8, 512 * 512, 128, 32) == 0
    assert L.gd_nn_groupnorm_silu_fused_supported(2, 64 * 64, 320, 32) == 0        # 10-channel runs: two-pass is level
    assert L.gd_nn_groupnorm_silu_fused_supported(2, 64, 328, 41) == 1             # C / G = 8
    assert L.gd_nn_groupnorm_silu_fused_supported(2, 64, 96, 32) == 0              # C / G odd
    assert L.gd_nn_groupnorm_silu_fused_supported(2, 64, 64, 32) == 0              # C / G = 2
    x = torch.zeros(2, 640, 64, 64, device=DEV, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = torch.ones(640, device=DEV, dtype=torch.bfloat16)
    ret = L.gd_nn_groupnorm_silu_fused_forward(torch.cuda.current_stream().cuda_stream, x.data_ptr(), x.data_ptr(), w.data_ptr(),
                                               w.data_ptr(), 2, 64 * 64, 640, 32, 1e-5, 1)
    assert ret == -1 and b"fused GroupNorm" in L.gd_nn_last_error()
    with torch.no_grad():          # the dispatch falls back to the two-pass kernels
        y = nn_ops.group_norm_silu(torch.randn_like(x), w, torch.zeros_like(w), 32, 1e-5, True)
    assert torch.isfinite(y.float()).all()

@pytest.mark.parametrize("N,C,H,W,silu", [(1, 640, 32, 32, True), (2, 960, 32, 32, True), (2, 1280, 32, 32, True),
                                          (1, 1920, 32, 32, False), (2, 1280, 16, 16, True), (1, 2560, 16, 16, True),
                                          (2, 1280, 8, 8, False), (1, 1920, 5, 7, True), (2, 128, 2, 2, True)])
def test_one_launch_groupnorm_training_pair_matches_fp32_reference_and_the_two_pass_kernels(N, C, H, W, silu):
    """GroupNorm(+SiLU) WITH an input gradient on the LoRA UNet's training maps: one launch forward that keeps mean / rstd
    (gd_nn_groupnorm_silu_fused_forward_stats) and one launch backward with x and dy of the (image, group) slice in registers
    (gd_nn_groupnorm_silu_fused_backward; slices above 32768 elements take the two-pass backward on the kept statistics) --
    against fp32 torch at the GroupNorm bars and against the two-pass pair; bit-reproducible."""
    from garmentdreamer_amd import nn_ops
    L = nn_ops.lib()
    assert L.gd_nn_groupnorm_silu_fused_supported(N, H * W, C, 32) == 1
    assert L.gd_nn_groupnorm_silu_fused_backward_supported(N, H * W, C, 32) == (1 if H * W * (C // 64) <= 16384 else 0)
    g = torch.Generator(DEV).manual_seed(C + H + N)
    x = (torch.randn(N, C, H, W, device=DEV, generator=g) * 1.7 + 0.4).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(C, device=DEV, generator=g) * 0.5 + 1.0).to(torch.bfloat16)
    b = (torch.randn(C, device=DEV, generator=g) * 0.3).to(torch.bfloat16)
    gy = torch.randn(N, C, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    outs = []
    for fn in (lambda t: nn_ops.group_norm_silu(t, w, b, 32, 1e-5, silu), lambda t: nn_ops.group_norm_silu(t, w, b, 32, 1e-5, silu),
               lambda t: nn_ops._GroupNormSiLU.apply(t, w, b, 32, 1e-5, silu)):
        xi = x.detach().clone().requires_grad_(True)
        y = fn(xi)
        y.backward(gy)
        outs.append((y.detach(), xi.grad, type(y.grad_fn).__name__))
    (y, dx, name), (y_again, dx_again, _), (y2, dx2, name2) = outs
    assert "GroupNormSiLUSmall" in name and "GroupNormSiLUSmall" not in name2
    assert torch.equal(y, y_again) and torch.equal(dx, dx_again)
    with torch.no_grad():
        assert torch.equal(y, nn_ops.group_norm_silu(x, w, b, 32, 1e-5, silu))      # the inference launch, same bits
    xr = x.detach().float().requires_grad_(True)
    yr = F.group_norm(xr, 32, w.float(), b.float(), 1e-5)
    yr = F.silu(yr) if silu else yr
    yr.backward(gy.float())
    assert (y.float() - yr).abs().max().item() <= 2e-2 * yr.abs().max().item() + 1e-2
    gerr = (dx.float() - xr.grad).abs().max().item()
    assert gerr <= 2e-2 * xr.grad.abs().max().item() + 1e-3, gerr
    assert F.cosine_similarity(dx.float().flatten(), xr.grad.flatten(), dim=0).item() > 0.9995
    # vs the two-pass pair: statistics equal up to the last bit, so outputs / gradients differ by bf16 rounding steps at most
    assert (dx.float() - dx2.float()).abs().max().item() <= 2e-2 * xr.grad.abs().max().item() + 1e-3
    assert (dx.float() - xr.grad).abs().mean().item() <= 1.2 * (dx2.float() - xr.grad).abs().mean().item() + 1e-6


def test_groupnorm_workspace_is_shared_and_left_zero():
    """The statistics workspace is zero-initialised once per (device, stream) and every call must leave it zero
    (last-workgroup finalize + clear, include/gd_nn.h): interleave shapes, forward and backward, on one workspace,
    check each result against fp32 torch and the workspace bytes afterwards."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(5)
    shapes = [(8, 128, 64, 64), (1, 320, 16, 16), (16, 1280, 8, 8), (2, 512, 128, 128), (3, 640, 7, 9), (8, 128, 64, 64)]
    for rep in range(2):
        for (N, C, H, W) in shapes:
            x = (torch.randn(N, C, H, W, device=DEV, generator=g) * 1.3 - 0.2).to(torch.bfloat16) \
                .contiguous(memory_format=torch.channels_last).requires_grad_(True)
            w = (torch.randn(C, device=DEV, generator=g) * 0.5 + 1.0).to(torch.bfloat16)
            b = (torch.randn(C, device=DEV, generator=g) * 0.3).to(torch.bfloat16)
            y = nn_ops.group_norm_silu(x, w, b, 32, 1e-6, True)
            gy = torch.randn(N, C, H, W, device=DEV, generator=g).to(torch.bfloat16)
            y.backward(gy)
            xr = x.detach().float().requires_grad_(True)
            yr = F.silu(F.group_norm(xr, 32, w.float(), b.float(), 1e-6))
            yr.backward(gy.float())
            assert (y.float() - yr).abs().max().item() <= 2e-2 * yr.abs().max().item() + 1e-2
            assert F.cosine_similarity(x.grad.float().flatten(), xr.grad.flatten(), dim=0).item() > 0.9995
    torch.cuda.synchronize()
    assert len(nn_ops._gn_ws_cache) >= 1
    for ws in nn_ops._gn_ws_cache.values():
        assert int(ws.count_nonzero()) == 0


def test_batched_time_embedding_projection_equals_per_block_projection():
    """UNet2DConditionModel._project_temb: one GEMM over the concatenated time_emb_proj weights (strided per-image
    bias handed to the conv kernels) vs every ResnetBlock2D projecting for itself -- same network output up to the
    bf16 rounding of the two GEMM shapes; and the per-block path is what runs when the embedding needs a gradient."""
    from garmentdreamer_amd.guidance import sd21
    with torch.device(DEV):
        unet = sd21.init_random_(sd21.UNet2DConditionModel(block_out_channels=(64, 128, 256, 256),
                                                           attention_head_dim=(1, 2, 4, 4)))
    unet = unet.to(torch.bfloat16).to(memory_format=torch.channels_last).eval()
    for p_ in unet.parameters():
        p_.requires_grad_(False)
    g = torch.Generator(DEV).manual_seed(3)
    x = torch.randn(3, 4, 32, 32, device=DEV, generator=g).to(torch.bfloat16)
    ctx = torch.randn(3, 77, 1024, device=DEV, generator=g).to(torch.bfloat16)
    t = torch.tensor([17.0, 480.0, 977.0], device=DEV)
    with torch.no_grad():
        y_batched = unet(x, t, encoder_hidden_states=ctx)
        packed = unet._project_temb(torch.randn(3, 256, device=DEV).to(torch.bfloat16))
        assert isinstance(packed, sd21.TembProjections) and len(packed.image_bias) == 22
        orig = unet._project_temb
        unet._project_temb = lambda temb: temb
        y_blocks = unet(x, t, encoder_hidden_states=ctx)
        unet._project_temb = orig
    scale = y_blocks.float().abs().max().item()
    assert (y_batched.float() - y_blocks.float()).abs().max().item() <= 3e-2 * scale
    assert F.cosine_similarity(y_batched.float().flatten(), y_blocks.float().flatten(), dim=0).item() > 0.9995
    # the other launch-count reductions of the frozen no-grad path (cross-attention K/V of the text embeddings from
    # one GEMM, feed-forward residual inside the GEMM with its bias folded into proj_out, fused QKV, own attention)
    # against the plain per-layer path, which is what runs with autograd on
    with torch.no_grad():
        ctxp = unet._project_context(ctx)
    assert isinstance(ctxp, sd21.ContextProjections) and len(ctxp.kv) == 16
    assert unet._project_context(ctx) is ctx          # autograd on: every layer projects for itself
    with torch.enable_grad():
        unet._project_temb = lambda temb: temb
        y_plain = unet(x, t, encoder_hidden_states=ctx).detach()
        unet._project_temb = orig
    assert (y_batched.float() - y_plain.float()).abs().max().item() <= 4e-2 * scale
    assert F.cosine_similarity(y_batched.float().flatten(), y_plain.float().flatten(), dim=0).item() > 0.999
    temb = torch.randn(3, 256, device=DEV).to(torch.bfloat16).requires_grad_(True)
    # gradient wanted (LoRA / camera embedding training): still ONE GEMM since round 5, under autograd, split views per block
    packed = unet._project_temb(temb)
    assert isinstance(packed, sd21.TembProjections) and all(v.requires_grad for v in packed.image_bias.values())


def test_training_time_embedding_as_one_gemm_and_bias_gradient_inside_the_conv_node(monkeypatch):
    """Round 5, NeTF stage: with the camera / shading embedding training, the 22 ``time_emb_proj`` of the LoRA UNet run as ONE GEMM
    under autograd (split views per block; backward = one concatenation + one GEMM + one SiLU backward) and each conv1 takes its
    per-image bias in the kernel epilogue, the autograd node returning the bias gradient -- instead of 22 x (SiLU, GEMM, two adds)
    forward and 22 x (pixel sum, GEMM, SiLU backward, accumulation) backward.  Same network output and same gradients for the camera
    MLP, the shading embedding and the adapters as the per-block path, to the bf16 rounding of the two forms, and against fp32
    eager on the same weights."""
    from garmentdreamer_amd.guidance import sd21
    kw = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4))
    with torch.device(DEV):
        lora = sd21.init_random_(sd21.LoraUNet2DConditionModel(**kw), 2)
        g = torch.Generator(DEV).manual_seed(11)
        for layer in lora.lora_layers:                        # non-zero up-projections: the adapter gradients carry signal
            for m in layer.values():
                m.up.weight.data.normal_(0, 0.02, generator=g)
    import copy
    ref = copy.deepcopy(lora).float()
    ref_train = ref.freeze_base()
    lora = lora.to(torch.bfloat16).to(memory_format=torch.channels_last)
    lora.trainables_to_fp32()
    train = lora.freeze_base()
    x = torch.randn(2, 4, 32, 32, device=DEV, generator=g)
    ctx = torch.randn(2, 77, 1024, device=DEV, generator=g)
    pose = torch.randn(2, 16, device=DEV, generator=g)
    t = torch.tensor([317.0, 611.0], device=DEV)
    wgt = torch.randn(2, 4, 32, 32, device=DEV, generator=g)

    def run(net, params, dtype):
        for p_ in params:
            p_.grad = None
        y = net(x.to(dtype), t, ctx.to(dtype), c=pose, shading="lambertian")
        (y.float() * wgt).sum().backward()
        names = {id(p_): n for n, p_ in net.named_parameters()}
        return y.detach().float(), {names[id(p_)]: p_.grad.detach().float().clone() for p_ in params if p_.grad is not None}

    monkeypatch.setattr(sd21, "_TEMB_TRAIN_CAT", False)
    monkeypatch.setattr(sd21, "_CONV_BIAS_GRAD", False)
    y_old, g_old = run(lora, train, torch.bfloat16)
    monkeypatch.setattr(sd21, "_TEMB_TRAIN_CAT", True)
    monkeypatch.setattr(sd21, "_CONV_BIAS_GRAD", True)
    y_new, g_new = run(lora, train, torch.bfloat16)
    y_ref, g_ref = run(ref, ref_train, torch.float32)
    cos = lambda a, b: F.cosine_similarity(a.flatten(), b.flatten(), dim=0).item()
    assert cos(y_new, y_old) > 0.9995 and cos(y_new, y_ref) > 0.999
    assert set(g_new) == set(g_old) == set(g_ref)
    emb = [n for n in g_new if n.startswith("camera_emb") or n.endswith("_emb")]
    assert len(emb) == 5                                    # the camera MLP's four tensors + the lambertian embedding
    for n in emb:
        assert cos(g_new[n], g_ref[n]) > 0.99, (n, cos(g_new[n], g_ref[n]), cos(g_old[n], g_ref[n]))
        assert cos(g_new[n], g_old[n]) > 0.99, (n, cos(g_new[n], g_old[n]))
    lo = [n for n in g_new if "lora" in n]
    cat = lambda d: torch.cat([d[n].flatten() for n in lo])
    assert cos(cat(g_new), cat(g_ref)) > 0.995 and cos(cat(g_new), cat(g_old)) > 0.995


@pytest.mark.parametrize("N,cin,cout,H,W", [(8, 128, 128, 128, 128), (2, 128, 256, 32, 32), (1, 256, 256, 24, 40)])
def test_vae_resnet_block_as_one_autograd_node_matches_fp32_reference(N, cin, cout, H, W):
    """nn_ops._ResnetBlockFrozen (VAE ResnetBlock2D, skip gradient summed inside the GroupNorm backward) against
    the same block in fp32 torch ops: output and input gradient; both the fused GN-conv maps and the small ones,
    with and without the 1x1 shortcut."""
    from garmentdreamer_amd import nn_ops
    from garmentdreamer_amd.guidance import sd21
    torch.manual_seed(cin + cout + H)
    with torch.device(DEV):
        blk32 = sd21.ResnetBlock2D(cin, cout, None, eps=1e-6)
        for p_ in blk32.parameters():
            p_.data.normal_(0.0, 0.05)
        blk32.norm1.weight.data.add_(1.0)
        blk32.norm2.weight.data.add_(1.0)
    blk = sd21.ResnetBlock2D(cin, cout, None, eps=1e-6).to(DEV)
    blk.load_state_dict(blk32.state_dict())
    blk = blk.to(torch.bfloat16).to(memory_format=torch.channels_last)
    for p_ in list(blk.parameters()) + list(blk32.parameters()):
        p_.requires_grad_(False)
    blk32.load_state_dict({k: v.float() for k, v in blk.state_dict().items()})     # identical (bf16-rounded) weights
    g = torch.Generator(DEV).manual_seed(1)
    x = torch.randn(N, cin, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(N, cout, H, W, device=DEV, generator=g).to(torch.bfloat16)
    xb = x.clone().requires_grad_(True)
    assert nn_ops.resnet_block_frozen_supported(xb, blk)
    y = blk(xb)
    assert y.grad_fn is not None and "ResnetBlockFrozen" in type(y.grad_fn).__name__
    y.backward(gy)
    xr = x.float().requires_grad_(True)
    yr = blk32(xr)
    yr.backward(gy.float())
    assert (y.float() - yr).abs().max().item() <= 3e-2 * yr.abs().max().item() + 1e-2
    assert F.cosine_similarity(y.float().flatten(), yr.flatten(), dim=0).item() > 0.9995
    assert (xb.grad.float() - xr.grad).abs().max().item() <= 4e-2 * xr.grad.abs().max().item()
    assert F.cosine_similarity(xb.grad.float().flatten(), xr.grad.flatten(), dim=0).item() > 0.999


@pytest.mark.parametrize("N,cin,cout,H,W,res", [(2, 128, 128, 256, 256, False),   # GroupNorm-in-loader kernel, BN = 128
                                                (1, 128, 256, 512, 256, True),    # ... BN = 256
                                                (8, 256, 512, 64, 64, True),      # persistent plain kernel, BN = 256
                                                (3, 128, 128, 250, 270, True),    # ragged: edge tiles, fused
                                                (5, 192, 384, 100, 75, False)])   # ragged, persistent, BN = 128
def test_groupnorm_statistics_from_the_conv_epilogue_match_the_statistics_pass(N, cin, cout, H, W, res):
    """gd_nn_conv3x3_*_stats + gd_nn_groupnorm_finish_partials: mean / rstd of the convolution's OUTPUT as left by
    its epilogue against gd_nn_groupnorm_stats run over that output, and against fp64 torch; the output itself is
    bit-identical with and without the statistics; two launches give bit-identical statistics (no atomics)."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(N * 1000 + H)
    cl = torch.channels_last
    x = (torch.randn(N, cin, H, W, device=DEV, generator=g) * 1.5 + 0.3).to(torch.bfloat16).contiguous(memory_format=cl)
    w = (torch.randn(cout, cin, 3, 3, device=DEV, generator=g) * 0.03).to(torch.bfloat16).contiguous(memory_format=cl)
    b = torch.randn(cout, device=DEV, generator=g).to(torch.bfloat16)
    gw = (1 + 0.1 * torch.randn(cin, device=DEV, generator=g)).to(torch.bfloat16)
    gb = (0.1 * torch.randn(cin, device=DEV, generator=g)).to(torch.bfloat16)
    r = torch.randn(N, cout, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=cl) if res else None
    groups, eps = 32, 1e-6
    y0, mr0, none = nn_ops._gnconv_forward(x, gw, gb, groups, eps, w, b, r)
    assert none is None
    y1, mr1, mrn = nn_ops._gnconv_forward(x, gw, gb, groups, eps, w, b, r, next_norm=(groups, eps))
    assert mrn is not None, "this shape should run on a patch-staged kernel"
    assert torch.equal(y0, y1) and torch.equal(mr0, mr1)
    y2, _, mrn2 = nn_ops._gnconv_forward(x, gw, gb, groups, eps, w, b, r, mr=mr1, next_norm=(groups, eps))
    assert torch.equal(y1, y2) and torch.equal(mrn, mrn2)
    ws = nn_ops._gn_workspace(y1, N, groups)
    ref = torch.empty_like(mrn)
    nn_ops._check(nn_ops.lib().gd_nn_groupnorm_stats(torch.cuda.current_stream().cuda_stream, y1.data_ptr(), N, H * W, cout,
                                                     groups, eps, ws.data_ptr(), ref.data_ptr()), "gd_nn_groupnorm_stats")
    yd = y1.double().reshape(N, groups, cout // groups, H * W)
    mean64, var64 = yd.mean(dim=(2, 3)), yd.var(dim=(2, 3), unbiased=False)
    got = mrn.view(N, groups, 2).double()
    assert torch.allclose(got[..., 0], mean64, rtol=1e-5, atol=1e-6)
    assert torch.allclose(got[..., 1], (var64 + eps).rsqrt(), rtol=1e-5)
    assert torch.allclose(mrn, ref, rtol=2e-6, atol=1e-7)


def test_statistics_riding_on_a_tensor_are_dropped_when_the_tensor_changes():
    """``_gd_gn_stats`` (statistics a producer left on its output) is only honoured for the very tensor version and
    GroupNorm configuration it was made for: an in-place edit of the tensor, or a consumer with other groups / eps,
    falls back to a statistics pass -- same result as without any riding statistics."""
    from garmentdreamer_amd import nn_ops
    from garmentdreamer_amd.guidance import sd21
    torch.manual_seed(11)
    with torch.device(DEV):
        b1 = sd21.init_random_(sd21.ResnetBlock2D(128, 128, None, eps=1e-6))
        b2 = sd21.init_random_(sd21.ResnetBlock2D(128, 128, None, eps=1e-6))
        b3 = sd21.init_random_(sd21.ResnetBlock2D(128, 128, None, eps=1e-5))
    for b in (b1, b2, b3):
        b.to(torch.bfloat16).to(memory_format=torch.channels_last)
        for p_ in b.parameters():
            p_.requires_grad_(False)
    x = torch.randn(2, 128, 256, 256, device=DEV).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    x.requires_grad_(True)
    y = b1(x, next_norm=b2.norm1)
    assert getattr(y, "_gd_gn_stats", None) is not None
    ref_same = b2(y.detach().clone().requires_grad_(True))          # no riding statistics: own pass
    got_same = b2(y)                                                  # riding statistics
    assert F.cosine_similarity(ref_same.float().flatten(), got_same.float().flatten(), dim=0).item() > 0.99999
    # another eps: the tag does not match, the consumer runs its own pass -> bit-identical to the untagged call
    assert torch.equal(b3(y), b3(y.detach().clone().requires_grad_(True)))
    # in-place edit: the version counter moved on, the stale statistics must not be used
    with torch.no_grad():
        y2 = y.detach().clone()
        y2._gd_gn_stats = y._gd_gn_stats[:3] + (y2._version,)
        y2.mul_(3.0)
    y2.requires_grad_(True)
    assert torch.equal(b2(y2), b2(y2.detach().clone().requires_grad_(True)))


def test_vae_encoder_with_epilogue_statistics_equals_the_statistics_pass_path(monkeypatch):
    """The VAE encoder with GroupNorm statistics riding on the tensors (conv epilogue -> next GroupNorm) against the
    same encoder with a statistics pass per GroupNorm: latents and image gradient agree to bf16 rounding noise, and
    the fast path really skipped the passes (counted at the C-ABI)."""
    from garmentdreamer_amd import nn_ops
    from garmentdreamer_amd.guidance import sd21
    torch.manual_seed(3)
    vae = sd21.AutoencoderKLEncoder().to(DEV).to(torch.bfloat16).to(memory_format=torch.channels_last)
    for p_ in vae.parameters():
        p_.requires_grad_(False)
    g = torch.Generator(DEV).manual_seed(5)
    img = torch.rand(4, 3, 256, 256, device=DEV, generator=g).to(torch.bfloat16)
    gy = torch.randn(4, 4, 32, 32, device=DEV, generator=g).to(torch.bfloat16)

    L = nn_ops.lib()
    passes = {"n": 0}
    real_stats, real_fwd = L.gd_nn_groupnorm_stats, L.gd_nn_groupnorm_silu_forward

    def counted_stats(*a):
        passes["n"] += 1
        return real_stats(*a)

    def counted_fwd(*a):
        passes["n"] += a[11] is not None      # stats_ws given: the call runs its own statistics pass
        return real_fwd(*a)

    real_small = L.gd_nn_groupnorm_silu_fused_forward_stats

    def counted_small(*a):                    # the one-launch form of small maps forms its own statistics too
        passes["n"] += 1
        return real_small(*a)

    monkeypatch.setattr(L, "gd_nn_groupnorm_stats", counted_stats)
    monkeypatch.setattr(L, "gd_nn_groupnorm_silu_forward", counted_fwd)
    monkeypatch.setattr(L, "gd_nn_groupnorm_silu_fused_forward_stats", counted_small)

    def run(flag):
        monkeypatch.setattr(nn_ops, "_EPILOGUE_STATS", flag)
        passes["n"] = 0
        x = img.clone().requires_grad_(True)
        z = vae.encode(x * 2 - 1).latent_dist.mean
        z.backward(gy)
        return z.detach().float(), x.grad.detach().float(), passes["n"]

    z0, g0, n0 = run(False)
    z1, g1, n1 = run(True)
    # 11 ResnetBlock2D = 22 GroupNorms (+ mid attention + conv_norm_out); with 4 images of 256^2 the two top levels run
    # on the patch-staged kernels: norm2 of both blocks and norm1 of the second block, per level, ride on the tensors
    # ... and norm1 of the very first block takes them from conv_in
    assert n0 >= 22 and n1 == n0 - 7, (n0, n1)
    assert F.cosine_similarity(z0.flatten(), z1.flatten(), dim=0).item() > 0.9999
    assert F.cosine_similarity(g0.flatten(), g1.flatten(), dim=0).item() > 0.999
    assert (z0 - z1).abs().max().item() <= 2e-2 * z0.abs().max().item()


def test_unet_and_vae_bf16_hip_path_tracks_fp32_torch_path():
    """Whole small UNet / VAE: bf16 + HIP GroupNorm kernels vs the same weights in fp32 torch ops."""
    from garmentdreamer_amd.guidance import sd21
    with torch.device(DEV):
        unet = sd21.init_random_(sd21.UNet2DConditionModel(block_out_channels=(64, 128, 256, 256),
                                                           attention_head_dim=(1, 2, 4, 4)))
        vae = sd21.init_random_(sd21.AutoencoderKLEncoder(block_out_channels=(32, 64, 128, 128)))
    for p in list(unet.parameters()) + list(vae.parameters()):
        p.requires_grad_(False)   # the guidance freezes every weight (stable_diffusion_guidance.py:99-102)
    x = torch.randn(2, 4, 32, 32, device=DEV)
    t = torch.tensor([50, 800], device=DEV)
    c = torch.randn(2, 77, 1024, device=DEV)
    with torch.no_grad():
        y32 = unet(x, t, c)
        y16 = unet.to(torch.bfloat16).to(memory_format=torch.channels_last)(x, t, c).float()
    cos = F.cosine_similarity(y32.flatten(), y16.flatten(), dim=0).item()
    assert cos > 0.995, cos
    img = torch.rand(2, 3, 128, 128, device=DEV)
    i32 = img.clone().requires_grad_(True)
    l32 = vae.encode(i32).latent_dist.mode()
    l32.square().sum().backward()
    vae16 = vae.to(torch.bfloat16).to(memory_format=torch.channels_last)
    i16 = img.clone().requires_grad_(True)
    l16 = vae16.encode(i16).latent_dist.mode().float()
    l16.square().sum().backward()
    assert F.cosine_similarity(l32.flatten(), l16.flatten(), dim=0).item() > 0.995
    assert F.cosine_similarity(i32.grad.flatten(), i16.grad.flatten(), dim=0).item() > 0.98


@pytest.mark.parametrize("N,Cin,H,W", [(2, 3, 64, 64), (1, 3, 37, 53), (3, 1, 16, 16), (1, 2, 129, 17), (8, 3, 128, 128)])
def test_first_conv_input_gradient_reads_dy_once_and_matches_fp32_reference(N, Cin, H, W, monkeypatch):
    """csrc/nn_conv_first_dgrad.h (round 5): input gradient of the VAE's first convolution as a 128 -> 9 x Cin product per pixel +
    the nine shifted sums through LDS.  Against fp32 autograd of F.conv2d on the same bf16 operands and against the padded
    implicit-GEMM form it replaced; ragged tiles (image edges inside a 16x16 tile), 1-3 channels, asymmetric data."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(17 * N + Cin + H)
    w = (torch.randn(128, Cin, 3, 3, device=DEV, generator=g) / 3).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    b = torch.randn(128, device=DEV, generator=g).to(torch.bfloat16)
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g).to(torch.bfloat16)
    dy = torch.randn(N, 128, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    assert nn_ops.lib().gd_nn_conv3x3_first_dgrad_supported(N, H, W, Cin, 128)
    out = {}
    for new in (True, False):
        monkeypatch.setattr(nn_ops, "_FIRST_DGRAD", new)
        xi = x.clone().requires_grad_(True)
        y = nn_ops.conv3x3_small_cin(xi, w, b)
        y.backward(dy)
        out[new] = xi.grad.float()
    x32 = x.float().requires_grad_(True)
    F.conv2d(x32, w.float(), b.float(), padding=1).backward(dy.float())
    ref = x32.grad
    scale = ref.abs().max().item()
    for new in (True, False):
        err = (out[new] - ref).abs().max().item()
        assert err <= 1.5e-2 * scale, (new, err, scale)
        assert F.cosine_similarity(out[new].flatten(), ref.flatten(), dim=0).item() > 0.9999
    # fp32 accumulation of all 9 x 128 terms, one rounding: at least as close as the form it replaces
    assert (out[True] - ref).abs().max().item() <= (out[False] - ref).abs().max().item() + 4e-3 * scale


@pytest.mark.parametrize("N,Cin,Cout,H,W,per_image_bias,res", [
    (2, 64, 128, 16, 16, False, False), (1, 128, 128, 32, 40, False, True), (3, 320, 320, 16, 16, True, True),
    (2, 192, 64, 9, 13, True, False), (1, 64, 8, 16, 16, False, False), (2, 640, 320, 8, 8, False, True),
    (8, 128, 128, 64, 64, False, True), (2, 320, 320, 64, 64, True, True), (16, 1280, 1280, 8, 8, True, False)])
@pytest.mark.parametrize("split", [-1, 1, 2, 7])
def test_conv3x3_mfma_matches_fp32_reference(N, Cin, Cout, H, W, per_image_bias, res, split):
    """Asymmetric random data (catches operand / C-layout transposes), halo zero padding, ragged
    pixel and channel tiles, fused per-image bias and residual; plus the input gradient.  split = -1: the
    library's heuristic (the small shapes here run split over ranges of the (tap, channel step) sequence);
    1: never split; 2, 7: forced range counts that cut taps in the middle and leave ragged last ranges."""
    from garmentdreamer_amd.nn_ops import conv3x3, conv3x3_supported, lib
    lib().gd_nn_conv_force_split(split)
    try:
        _conv3x3_case(N, Cin, Cout, H, W, per_image_bias, res)
    finally:
        lib().gd_nn_conv_force_split(-1)


def _conv3x3_case(N, Cin, Cout, H, W, per_image_bias, res):
    from garmentdreamer_amd.nn_ops import conv3x3, conv3x3_supported
    g = torch.Generator(DEV).manual_seed(Cin * 7 + Cout)
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (3 * Cin ** 0.5)).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    b = torch.randn((N, Cout) if per_image_bias else (Cout,), device=DEV, generator=g).to(torch.bfloat16)
    r = torch.randn(N, Cout, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last) if res else None
    assert conv3x3_supported(x, w)
    xg = x.clone().requires_grad_(True)
    y = conv3x3(xg, w, b, r)
    xr = x.float().requires_grad_(True)
    yr = F.conv2d(xr, w.float(), None, padding=1) + (b.float()[:, :, None, None] if per_image_bias else b.float()[None, :, None, None])
    if res:
        yr = yr + r.float()
    assert y.shape == yr.shape and y.dtype == torch.bfloat16
    err = (y.float() - yr).abs().max().item()
    assert err <= 1.5e-2 * yr.abs().max().item() + 1e-2, err
    assert F.cosine_similarity(y.float().flatten(), yr.flatten(), dim=0).item() > 0.9999
    gy = torch.randn(y.shape, device=DEV, generator=g).to(torch.bfloat16)
    y.backward(gy)
    yr.backward(gy.float())
    gerr = (xg.grad.float() - xr.grad).abs().max().item()
    assert gerr <= 2e-2 * xr.grad.abs().max().item() + 1e-2, gerr
    assert F.cosine_similarity(xg.grad.float().flatten(), xr.grad.flatten(), dim=0).item() > 0.9995


def test_first_conv_small_cin_and_conv1x1_match_torch():
    from garmentdreamer_amd.nn_ops import conv1x1, conv3x3_small_cin
    g = torch.Generator(DEV).manual_seed(5)
    x = torch.rand(2, 3, 40, 56, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(128, 3, 3, 3, device=DEV, generator=g) / 5).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    b = torch.randn(128, device=DEV, generator=g).to(torch.bfloat16)
    xg = x.clone().requires_grad_(True)
    y = conv3x3_small_cin(xg, w, b)
    xr = x.float().requires_grad_(True)
    yr = F.conv2d(xr, w.float(), b.float(), padding=1)
    assert (y.float() - yr).abs().max().item() <= 2e-2 * yr.abs().max().item()
    gy = torch.randn(y.shape, device=DEV, generator=g).to(torch.bfloat16)
    y.backward(gy)
    yr.backward(gy.float())
    assert xg.grad.shape == x.shape
    assert F.cosine_similarity(xg.grad.float().flatten(), xr.grad.flatten(), dim=0).item() > 0.9995
    assert (xg.grad.float() - xr.grad).abs().max().item() <= 2e-2 * xr.grad.abs().max().item() + 1e-2
    # ragged row groups (W % 4 != 0), Cin = 4 (UNet conv_in), another Cout
    x4 = torch.rand(1, 4, 17, 53, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w4 = (torch.randn(320, 4, 3, 3, device=DEV, generator=g) / 6).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    b4 = torch.randn(320, device=DEV, generator=g).to(torch.bfloat16)     # 40 channel octets: 240 of 256 threads used
    with torch.no_grad():
        y4 = conv3x3_small_cin(x4, w4, b4)
        r4 = F.conv2d(x4.float(), w4.float(), b4.float(), padding=1)
    assert y4.shape == r4.shape and (y4.float() - r4).abs().max().item() <= 2e-2 * r4.abs().max().item()
    x1 = torch.randn(2, 256, 12, 20, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w1 = (torch.randn(128, 256, 1, 1, device=DEV, generator=g) / 16).to(torch.bfloat16)
    b1 = torch.randn(128, device=DEV, generator=g).to(torch.bfloat16)
    y1 = conv1x1(x1, w1, b1)
    r1 = F.conv2d(x1.float(), w1.float(), b1.float())
    assert y1.shape == r1.shape and y1.is_contiguous(memory_format=torch.channels_last)
    assert (y1.float() - r1).abs().max().item() <= 2e-2 * r1.abs().max().item()


@pytest.mark.parametrize("N,cin,H,W,with_bias", [(2, 3, 40, 56, True), (1, 3, 512, 512, True), (3, 4, 33, 100, False),
                                                  (2, 1, 7, 31, True), (1, 2, 64, 32, True)])
def test_first_conv_on_the_matrix_cores_and_its_groupnorm_statistics(N, cin, H, W, with_bias):
    """gd_nn_conv3x3_first_forward for Cout = 128 (im2col gathered per lane, bias as a K column) against fp32 torch --
    to one bf16 rounding of the result, since products of bf16 values and their fp32 sums are what torch computes
    too -- and the epilogue's GroupNorm statistics against fp64 statistics of the stored tensor."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(N + 10 * cin + H)
    cl = torch.channels_last
    x = (torch.rand(N, cin, H, W, device=DEV, generator=g) * 2 - 1).to(torch.bfloat16).contiguous(memory_format=cl)
    w = (torch.randn(128, cin, 3, 3, device=DEV, generator=g) / 4).to(torch.bfloat16).contiguous(memory_format=cl)
    b = torch.randn(128, device=DEV, generator=g).to(torch.bfloat16) if with_bias else None
    y, mrn = nn_ops._ConvSmallCin.apply(x, w, b, (32, 1e-6))
    y_plain, none = nn_ops._ConvSmallCin.apply(x, w, b, None)
    assert none is None and torch.equal(y, y_plain)
    ref = F.conv2d(x.float(), w.float(), None if b is None else b.float(), padding=1)
    assert (y.float() - ref).abs().max().item() <= 2.0 ** -8 * ref.abs().max().item()
    assert mrn is not None
    yd = y.double().reshape(N, 32, 4, H * W)
    got = mrn.view(N, 32, 2).double()
    assert torch.allclose(got[..., 0], yd.mean(dim=(2, 3)), rtol=1e-5, atol=1e-6)
    assert torch.allclose(got[..., 1], (yd.var(dim=(2, 3), unbiased=False) + 1e-6).rsqrt(), rtol=1e-5)
    _, mrn2 = nn_ops._ConvSmallCin.apply(x, w, b, (32, 1e-6))
    assert torch.equal(mrn, mrn2)


def test_vsd_step_runs_through_hip_kernels_with_lora_backward():
    """NeTF VSD iteration on the GPU with small networks: guidance step (grad reaches the image) and the
    LoRA training step (grads reach only adapters / camera MLP) through the MFMA conv + GroupNorm kernels."""
    from garmentdreamer_amd.guidance import sd21
    from garmentdreamer_amd.guidance.sd_vsd import LoraUnet, StableDiffusionVSD
    kw = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4))
    with torch.device(DEV):
        unet = sd21.init_random_(sd21.UNet2DConditionModel(**kw))
        vae = sd21.init_random_(sd21.AutoencoderKLEncoder(block_out_channels=(64, 64, 128, 128)))
        lora = sd21.init_random_(sd21.LoraUNet2DConditionModel(**kw), 3)
    gd = StableDiffusionVSD(DEV, fp16=True, unet=unet, vae=vae)
    lora = lora.to(torch.bfloat16).to(memory_format=torch.channels_last)
    train = lora.freeze_base()
    q = LoraUnet(lora)
    gd.set_text_embeds(torch.randn(1, 77, 1024, device=DEV), torch.randn(1, 77, 1024, device=DEV))
    img = torch.rand(1, 3, 512, 512, device=DEV, requires_grad=True)
    pose = torch.randn(1, 16, device=DEV)
    loss, pseudo, latents = gd.train_step(img, q_unet=q, pose=pose, shading="albedo")
    loss.backward()
    assert torch.isfinite(img.grad).all() and img.grad.abs().sum() > 0
    lu = gd.lora_train_loss(q, latents, pose, unet_bs=2, drop_pose=False)
    lu.backward()
    got = [n for n, p in lora.named_parameters() if p.grad is not None and p.grad.abs().sum() > 0]
    assert any("lora" in n for n in got) and any(n.startswith("camera_emb") for n in got)
    assert all(torch.isfinite(p.grad).all() for p in train if p.grad is not None)


def test_hip_graph_replay_matches_eager_guidance():
    """use_hip_graphs=True (UNet forward graph + VAE fwd/bwd graphs) gives the same loss and the same
    image gradient as eager launches, on repeated calls with changing inputs."""
    from garmentdreamer_amd.guidance import sd21
    from garmentdreamer_amd.guidance.stable_diffusion_guidance import PromptEmbeddings, StableDiffusionGuidance
    kw = dict(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4))
    with torch.device(DEV):
        unet = sd21.init_random_(sd21.UNet2DConditionModel(**kw))
        vae = sd21.init_random_(sd21.AutoencoderKLEncoder(block_out_channels=(64, 64, 128, 128)))
    prompt = PromptEmbeddings.random(DEV)
    outs = {}
    for graphs in (False, True):
        # guidance_scale 1: at the pipeline's scale of 100 the bf16 rounding noise of eps_text - eps_uncond
        # (1 ulp between two eager runs already) is amplified 100x and no longer says anything about graphs
        gd = StableDiffusionGuidance({"use_hip_graphs": graphs, "grad_clip": [0, 1.5, 2.0, 1000],
                                      "guidance_scale": 1.0}, device=DEV, unet=unet, vae=vae)
        gd.update_step(0, 0)
        res = []
        for it in range(3):
            g = torch.Generator(DEV).manual_seed(it)
            rgb = torch.rand(2, 64, 64, 3, device=DEV, generator=g).requires_grad_(True)
            out = gd(rgb, prompt, torch.tensor([10.0, 20.0], device=DEV), torch.tensor([0.0, 100.0], device=DEV),
                     torch.ones(2, device=DEV) * 2, noise=torch.randn(2, 4, 64, 64, device=DEV, generator=g),
                     timesteps=torch.tensor([100 + it, 700], device=DEV),
                     vae_noise=torch.randn(2, 4, 64, 64, device=DEV, generator=g))
            out["loss_sds"].backward()
            res.append((out["loss_sds"].item(), rgb.grad.clone()))
        outs[graphs] = res
    for (l0, g0), (l1, g1) in zip(outs[False], outs[True]):
        assert abs(l0 - l1) <= 2e-2 * abs(l0) + 1e-3, (l0, l1)
        assert F.cosine_similarity(g0.flatten(), g1.flatten(), dim=0).item() > 0.999


@pytest.mark.parametrize("rows,inner", [(4096, 1280), (777, 2560), (64, 5120), (3, 8)])
def test_geglu_matches_fp32_reference_and_eager_bf16(rows, inner):
    from garmentdreamer_amd.nn_ops import geglu
    g = torch.Generator(DEV).manual_seed(inner)
    x = (torch.randn(rows, 2 * inner, device=DEV, generator=g) * 2.0).to(torch.bfloat16)
    with torch.no_grad():
        y = geglu(x)
        h, gate = x.chunk(2, dim=-1)
        eager = h * F.gelu(gate)
        ref = h.float() * F.gelu(gate.float())
    assert y.shape == (rows, inner) and y.dtype == torch.bfloat16
    assert (y.float() - ref).abs().max().item() <= 1e-2 * ref.abs().max().item() + 1e-3   # two bf16 roundings
    # same rounding points as the eager bf16 ops -> (almost) bit-identical; allow 1 bf16 ulp for erf
    assert (y.float() - eager.float()).abs().max().item() <= 2 ** -7 * eager.float().abs().max().item()
    assert (y != eager).float().mean().item() < 1e-2


@pytest.mark.parametrize("rows,C,with_res", [(4096, 320, True), (1024, 640, True), (256, 1280, True), (64, 1280, False),
                                             (5, 2048, True), (7, 8, True)])
def test_add_layernorm_matches_fp32_reference(rows, C, with_res):
    from garmentdreamer_amd.nn_ops import add_layer_norm
    g = torch.Generator(DEV).manual_seed(C + rows)
    x = (torch.randn(rows, C, device=DEV, generator=g) * 1.5 + 0.3).to(torch.bfloat16)
    r = (torch.randn(rows, C, device=DEV, generator=g)).to(torch.bfloat16) if with_res else None
    norm = torch.nn.LayerNorm(C).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(torch.randn(C, device=DEV, generator=g) * 0.5 + 1.0)
        norm.bias.copy_(torch.randn(C, device=DEV, generator=g) * 0.3)
    norm = norm.to(torch.bfloat16)
    with torch.no_grad():
        s, y = add_layer_norm(x, r, norm)
        s_ref = x if r is None else x + r                     # the residual stream is bf16 in eager too
        y_ref = F.layer_norm(s_ref.float(), (C,), norm.weight.float(), norm.bias.float(), norm.eps)
    assert torch.equal(s, s_ref)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    err = (y.float() - y_ref).abs().max().item()
    assert err <= 1e-2 * y_ref.abs().max().item() + 1e-2, err    # one bf16 output rounding
    # with gradients required the wrapper must leave the autograd path intact
    x2 = x.clone().requires_grad_(True)
    s2, y2 = add_layer_norm(x2, r, norm)
    y2.float().sum().backward()
    assert x2.grad is not None and torch.isfinite(x2.grad).all()


@pytest.mark.parametrize("N,Cin,Cout,H,W,pad_lo", [(2, 128, 128, 32, 32, 0), (1, 256, 256, 17, 23, 0), (2, 320, 320, 16, 16, 1),
                                                   (1, 64, 192, 9, 14, 1), (3, 128, 64, 6, 5, 0), (1, 512, 512, 64, 64, 0),
                                                   (2, 1280, 1280, 16, 16, 1), (2, 640, 640, 32, 32, 1), (1, 320, 320, 64, 64, 1)])
def test_conv3x3_stride2_forward_and_dgrad_match_fp32_reference(N, Cin, Cout, H, W, pad_lo):
    """Downsample2D: UNet Conv2d(k3,s2,p1) (pad_lo 1) and the VAE's F.pad(0,1,0,1)+Conv2d(k3,s2,p0) (pad_lo 0)."""
    from garmentdreamer_amd.nn_ops import conv3x3_s2
    g = torch.Generator(DEV).manual_seed(Cin + H)
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (3 * Cin ** 0.5)).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    b = torch.randn(Cout, device=DEV, generator=g).to(torch.bfloat16)
    x.requires_grad_(True)
    y = conv3x3_s2(x, w, b, pad_lo)
    xr = x.detach().float().requires_grad_(True)
    xp = F.pad(xr, (pad_lo, 1, pad_lo, 1))
    yr = F.conv2d(xp, w.float(), b.float(), stride=2)
    assert y.shape == yr.shape and y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    err = (y.float() - yr).abs().max().item()
    assert err <= 1e-2 * yr.abs().max().item() + 1e-2, err
    gy = torch.randn(yr.shape, device=DEV, generator=g).to(torch.bfloat16)
    y.backward(gy)
    yr.backward(gy.float())
    assert x.grad.shape == x.shape
    gerr = (x.grad.float() - xr.grad).abs().max().item()
    assert gerr <= 1e-2 * xr.grad.abs().max().item() + 1e-3, gerr
    cos = F.cosine_similarity(x.grad.float().flatten(), xr.grad.flatten(), dim=0).item()
    assert cos > 0.9999, cos


@pytest.mark.parametrize("N,Cin,Cout,H,W,silu,per_image_bias,res", [
    (2, 128, 128, 32, 32, True, False, True), (1, 128, 256, 48, 40, True, False, False),
    (2, 320, 320, 16, 16, True, True, False), (1, 256, 256, 21, 19, False, False, True),
    (2, 512, 512, 16, 16, True, False, True), (1, 64, 64, 7, 9, True, False, False)])
def test_gn_conv3x3_fused_matches_fp32_reference(N, Cin, Cout, H, W, silu, per_image_bias, res):
    """conv3x3(silu(group_norm(x))) in one kernel (patch-staged, GroupNorm applied in the activation loader)."""
    from garmentdreamer_amd.nn_ops import gn_conv3x3
    g = torch.Generator(DEV).manual_seed(Cin + H + W)
    cl = torch.channels_last
    x = (torch.randn(N, Cin, H, W, device=DEV, generator=g) * 1.7 + 0.4).to(torch.bfloat16).contiguous(memory_format=cl)
    gw = (torch.randn(Cin, device=DEV, generator=g) * 0.5 + 1.0).to(torch.bfloat16)
    gb = (torch.randn(Cin, device=DEV, generator=g) * 0.3).to(torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (3 * Cin ** 0.5)).to(torch.bfloat16).contiguous(memory_format=cl)
    b = torch.randn((N, Cout) if per_image_bias else (Cout,), device=DEV, generator=g).to(torch.bfloat16)
    r = torch.randn(N, Cout, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=cl) if res else None
    x.requires_grad_(True)
    y = gn_conv3x3(x, gw, gb, 32, 1e-5, silu, w, b, r)
    xr = x.detach().float().requires_grad_(True)
    a = F.group_norm(xr, 32, gw.float(), gb.float(), 1e-5)
    a = F.silu(a) if silu else a
    yr = F.conv2d(a, w.float(), None if per_image_bias else b.float(), padding=1)
    if per_image_bias:
        yr = yr + b.float()[:, :, None, None]
    if res:
        yr = yr + r.float()
    assert y.shape == yr.shape and y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=cl)
    err = (y.float() - yr).abs().max().item()
    assert err <= 2e-2 * yr.abs().max().item() + 2e-2, err      # bf16 activations into the MFMA + bf16 output
    cos = F.cosine_similarity(y.float().flatten(), yr.flatten(), dim=0).item()
    assert cos > 0.9998, cos
    gy = torch.randn(yr.shape, device=DEV, generator=g).to(torch.bfloat16)
    y.backward(gy)
    yr.backward(gy.float())
    gcos = F.cosine_similarity(x.grad.float().flatten(), xr.grad.flatten(), dim=0).item()
    assert gcos > 0.999, gcos
    gerr = (x.grad.float() - xr.grad).abs().max().item()
    assert gerr <= 3e-2 * xr.grad.abs().max().item() + 1e-3, gerr


@pytest.mark.parametrize("N,Cin,Cout,H,W,per_image_bias,res", [(2, 128, 128, 64, 64, False, True), (1, 192, 320, 21, 19, True, False),
                                                             (3, 64, 64, 16, 16, False, False), (1, 256, 512, 40, 24, True, True),
                                                             (16, 320, 320, 64, 64, False, True)])
def test_plain_conv_on_patch_kernel_matches_fp32_reference(N, Cin, Cout, H, W, per_image_bias, res):
    """Plain 3x3 convolution on the patch-staged kernel (LDS-DMA patch): ragged patches, halo zero fill, both
    channel-slab widths; the last shape is one the library routes there by itself."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(Cin + Cout + H)
    cl = torch.channels_last
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (3 * Cin ** 0.5)).to(torch.bfloat16).contiguous(memory_format=cl)
    b = torch.randn((N, Cout) if per_image_bias else (Cout,), device=DEV, generator=g).to(torch.bfloat16)
    r = torch.randn(N, Cout, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=cl) if res else None
    yr = F.conv2d(x.float(), w.float(), None, padding=1) + (b.float()[:, :, None, None] if per_image_bias else b.float()[None, :, None, None])
    if res:
        yr = yr + r.float()
    for y in (nn_ops._patch_launch(x, w, b, r, Cout), nn_ops.conv3x3(x, w, b, r)):
        assert y.shape == yr.shape and y.is_contiguous(memory_format=cl)
        err = (y.float() - yr).abs().max().item()
        assert err <= 1.5e-2 * yr.abs().max().item() + 1e-2, err
        assert F.cosine_similarity(y.float().flatten(), yr.flatten(), dim=0).item() > 0.9999


@pytest.mark.parametrize("N,C,Cout,H,W", [(2, 128, 128, 16, 16), (1, 320, 320, 9, 13), (3, 64, 192, 5, 4), (2, 1280, 1280, 8, 8)])
def test_upsample_fused_conv_matches_fp32_reference(N, C, Cout, H, W):
    """gd_nn_conv3x3_up2_forward (four 2x2-tap convolutions with pre-summed filters) against
    conv2d(interpolate(x, 2, nearest)) in fp32 with the same bf16 weights; odd sizes exercise the borders."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(H * 31 + W)
    x = torch.randn(N, C, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, C, 3, 3, device=DEV, generator=g) * (1.0 / (3 * C ** 0.5))).to(torch.bfloat16) \
        .contiguous(memory_format=torch.channels_last)
    b = (torch.randn(Cout, device=DEV, generator=g) * 0.1).to(torch.bfloat16)
    with torch.no_grad():
        y = nn_ops.upsample2x_conv3x3(x, w, b)
        ref = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w.float(), b.float(), padding=1)
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    scale = ref.abs().max().item()
    assert (y.float() - ref).abs().max().item() <= 2e-2 * scale
    assert F.cosine_similarity(y.float().flatten(), ref.flatten(), dim=0).item() > 0.9998
    w2 = w.clone()                       # the pre-summed filters follow weight updates
    w2.mul_(0.5)
    with torch.no_grad():
        y2 = nn_ops.upsample2x_conv3x3(x, w2, None)
        ref2 = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w2.float(), None, padding=1)
    assert (y2.float() - ref2).abs().max().item() <= 2e-2 * ref2.abs().max().item()


def test_flipped_weight_cache_follows_weight_updates():
    """The dgrad weights are cached per weight tensor; loading new values in place (load_state_dict) must refresh them."""
    from garmentdreamer_amd.nn_ops import conv3x3
    cl = torch.channels_last
    g = torch.Generator(DEV).manual_seed(0)
    w = (torch.randn(64, 64, 3, 3, device=DEV, generator=g) * 0.05).to(torch.bfloat16).contiguous(memory_format=cl)
    x = torch.randn(2, 64, 16, 16, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    gy = torch.randn(2, 64, 16, 16, device=DEV, generator=g).to(torch.bfloat16)
    for _ in range(2):
        xg = x.clone().requires_grad_(True)
        conv3x3(xg, w, None, None).backward(gy)
        xr = x.float().requires_grad_(True)
        F.conv2d(xr, w.float(), padding=1).backward(gy.float())
        assert F.cosine_similarity(xg.grad.float().flatten(), xr.grad.flatten(), dim=0).item() > 0.9995
        with torch.no_grad():
            w.copy_((torch.randn(64, 64, 3, 3, device=DEV, generator=g) * 0.05).to(torch.bfloat16))   # "load_state_dict"


@pytest.mark.parametrize("B,H,S", [(2, 5, 4096), (3, 10, 1024), (2, 20, 256), (1, 3, 64), (2, 2, 192)])
def test_attention_d64_matches_fp32_reference(B, H, S):
    """Fused self-attention forward (head_dim 64): asymmetric random q / k / v (detects operand and key-order
    mix-ups), strided [B,S,H,64] views as the model passes them, plus a score spike that forces the running-maximum
    rescale branch after the first tiles."""
    from garmentdreamer_amd.nn_ops import attention_d64, attention_d64_supported
    g = torch.Generator(DEV).manual_seed(S + H)
    qkv = (torch.randn(B, S, 3 * H * 64, device=DEV, generator=g) * 1.5).to(torch.bfloat16)
    q, k, v = [t.view(B, S, H, 64) for t in qkv.chunk(3, dim=-1)]           # non-contiguous rows (stride 3*H*64)
    if S >= 256:   # one late key that dominates a few queries: m_run must move long after tile 0
        k = k.clone()
        k[:, S - 70, :, :] = (q[:, 5, :, :].float() * 3.0).to(torch.bfloat16)
    assert attention_d64_supported(q, k, v)
    with torch.no_grad():
        out = attention_d64(q, k, v)
        ref = F.scaled_dot_product_attention(q.transpose(1, 2).float(), k.transpose(1, 2).float(), v.transpose(1, 2).float())
        ref = ref.transpose(1, 2).reshape(B, S, H * 64)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    err = (out.float() - ref).abs().max().item()
    assert err <= 2e-2 * ref.abs().max().item() + 2e-3, err          # bf16 P and bf16 output
    assert F.cosine_similarity(out.float().flatten(), ref.flatten(), dim=0).item() > 0.9995
    if S % 64 == 0:
        # the entry that takes V already transposed ([B, H*64, S], e.g. W_v x^T from a GEMM): the same bits
        from garmentdreamer_amd.nn_ops import attention_d64_vt
        vt = v.reshape(B, S, H * 64).transpose(1, 2).contiguous()
        with torch.no_grad():
            out_vt = attention_d64_vt(q, k, vt)
        assert torch.equal(out_vt, out)


def test_full_size_sds_steps_stay_finite_with_hip_graphs():
    """Three iterations of the benchmark workload at 8 views with the real SD-2.1-sized networks and hipGraph replay
    of BOTH the UNet and the VAE: parameters and gradients must stay finite and the scene visible.  (A fast kernel
    path that silently produced NaN gradients once made every Gaussian vanish -- and the step look faster.)"""
    import argparse
    import bench
    from garmentdreamer_amd.gaussian_model import GaussianModel
    from garmentdreamer_amd.guidance.stable_diffusion_guidance import PromptEmbeddings, StableDiffusionGuidance
    from garmentdreamer_amd.scene import synthetic_gaussians
    from garmentdreamer_amd.sds_loop import SDSLoop
    dev = torch.device(DEV)
    V = 8
    args = argparse.Namespace(views=V, gaussians=20000, res=512)
    gm = GaussianModel.from_activated(synthetic_gaussians(20000, seed=0), device=dev)
    guid = StableDiffusionGuidance({"guidance_scale": 100.0, "grad_clip": [0, 1.5, 2.0, 1000], "use_hip_graphs": True}, device=dev)
    loop = SDSLoop(gm, guid, PromptEmbeddings.random(dev), torch.ones(3, device=dev))
    gen = torch.Generator(device=dev)
    for s in range(3):
        gen.manual_seed(100 + s)
        noise = torch.randn(V, 4, 64, 64, device=dev, generator=gen)
        vn = torch.randn(V, 4, 64, 64, device=dev, generator=gen)
        t = torch.randint(20, 981, (V,), device=dev, generator=gen)
        out = loop.step(bench.camera_batch(args, s, list(range(V))), noise=noise, timesteps=t, vae_noise=vn)
        assert torch.isfinite(out["loss"]).item()
        assert torch.isfinite(gm.flat_grad).all().item() and gm.flat_grad.abs().max().item() > 0
        assert torch.isfinite(gm._flat).all().item()
        assert int(out["num_visible"]) == 20000


@pytest.mark.parametrize("H,W", [(512, 512), (1024, 1024), (128, 128), (300, 420), (777, 600)])
def test_vae_prologue_matches_interpolate_affine_cast(H, W):
    """One launch each way == F.interpolate(bilinear, align_corners=False) * 2 - 1 -> bf16 NHWC and its autograd
    (stable_diffusion_guidance.py:394-396,164): identity size, the reference's 1024 -> 512, up-sampling, ragged."""
    from garmentdreamer_amd.nn_ops import vae_prologue, vae_prologue_supported
    g = torch.Generator(DEV).manual_seed(H + W)
    x = torch.rand(2, 3, H, W, device=DEV, generator=g)
    assert vae_prologue_supported(x)
    xa = x.clone().requires_grad_(True)
    ya = vae_prologue(xa, 512, 512)
    assert ya.shape == (2, 3, 512, 512) and ya.dtype == torch.bfloat16 and ya.is_contiguous(memory_format=torch.channels_last)
    xr = x.clone().requires_grad_(True)
    yr = F.interpolate(xr, (512, 512), mode="bilinear", align_corners=False) * 2.0 - 1.0
    assert (ya.float() - yr).abs().max().item() <= 2 ** -8 + 1e-6            # one bf16 rounding of values in [-1, 1]
    # gradient: a 4-channel NHWC gradient whose first three channels are the image's (the first conv's dgrad layout)
    gy4 = torch.randn(2, 4, 512, 512, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    ya.backward(gy4[:, :3])
    yr.backward(gy4[:, :3].float())
    scale = xr.grad.abs().max().item()
    assert (xa.grad - xr.grad).abs().max().item() <= 2e-6 * scale + 1e-6
    # ... and a plain contiguous 3-channel gradient
    xb = x.clone().requires_grad_(True)
    gy3 = torch.randn(2, 3, 512, 512, device=DEV, generator=g)
    vae_prologue(xb, 512, 512).backward(gy3)
    xc = x.clone().requires_grad_(True)
    (F.interpolate(xc, (512, 512), mode="bilinear", align_corners=False) * 2.0 - 1.0).backward(gy3.to(torch.bfloat16).float())
    assert (xb.grad - xc.grad).abs().max().item() <= 2e-6 * xc.grad.abs().max().item() + 1e-6


def test_sparsity_head_matches_torch_ops():
    """mean(sqrt((depth / (depth.max() + 1e-5))^2 + 0.01)) (GaussianDreamer.py:215,253): value, d/d depth and the
    gradient that flows through the maximum, against the torch expression."""
    from garmentdreamer_amd.nn_ops import sparsity_loss
    g = torch.Generator(DEV).manual_seed(3)
    d0 = torch.rand(4, 96, 160, 1, device=DEV, generator=g) * 3.0
    d0[1, 5, 7, 0] = 7.5     # a unique maximum
    da = d0.clone().requires_grad_(True)
    la = sparsity_loss(da, da.max())
    db = d0.clone().requires_grad_(True)
    lb = ((db / (db.max() + 1e-5)) ** 2 + 0.01).sqrt().mean()
    assert abs(la.item() - lb.item()) <= 1e-6 * abs(lb.item())
    (la * 3.0).backward()
    (lb * 3.0).backward()
    s = db.grad.abs().max().item()
    assert (da.grad - db.grad).abs().max().item() <= 1e-5 * s
    assert abs(da.grad[1, 5, 7, 0].item() - db.grad[1, 5, 7, 0].item()) <= 1e-4 * abs(db.grad[1, 5, 7, 0].item())


def _e4m3(x):
    """torch's own OCP e4m3fn conversion (round to nearest even) of an already clamped tensor -> (bytes, values)."""
    q = x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), q.float()


def test_fp8_quantize_and_pack_match_torch_e4m3fn():
    from garmentdreamer_amd.nn_ops import fp8_pack_weights, fp8_quantize
    g = torch.Generator(DEV).manual_seed(1)
    x = (torch.randn(3, 1000, 320, device=DEV, generator=g) * 40).to(torch.bfloat16)
    x[0, 0, :8] = torch.tensor([0.0, -0.0, 1e-4, 447.0, 449.0, -1000.0, 0.0019, 0.013], device=DEV).to(torch.bfloat16)
    s = 0.37
    q = fp8_quantize(x, s)
    ref, _ = _e4m3(x.float() * (1.0 / s))
    assert q.shape == x.shape and torch.equal(q, ref)
    w = (torch.randn(96, 320, device=DEV, generator=g)).to(torch.bfloat16)
    p = fp8_pack_weights(w, 0.02)
    assert p.shape == (96, 384)
    refw, _ = _e4m3(w.float() * (1.0 / 0.02))
    assert torch.equal(p[:, :320], refw) and int(p[:, 320:].max()) == 0


@pytest.mark.parametrize("M,K,N", [(4096, 320, 960), (65536, 320, 320), (1000, 1280, 10240), (16384, 2560, 640),
                                   (777, 640, 1284)])
def test_fp8_linear_matches_fp32_of_the_dequantised_operands(M, K, N):
    """The kernel's arithmetic: with the SAME e4m3 operands the fp32 reference agrees to accumulation rounding (catches
    every lane / byte / tile mix-up); asymmetric random A and B, ragged M and N, K that is not a multiple of 128."""
    from garmentdreamer_amd.nn_ops import fp8_linear, fp8_pack_weights, fp8_quantize
    g = torch.Generator(DEV).manual_seed(M + K + N)
    x = (torch.randn(M, K, device=DEV, generator=g) * 2.0).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g).to(torch.bfloat16)
    r = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    sx, sw = float(x.abs().max()) / 448.0, float(w.abs().max()) / 448.0
    x8, w8 = fp8_quantize(x, sx), fp8_pack_weights(w, sw)
    y = fp8_linear(x8, w8, b, r, K, sx * sw)
    _, xq = _e4m3(x.float() / sx)
    _, wq = _e4m3(w.float() / sw)
    ref = (xq @ wq.t()) * (sx * sw) + b.float() + r.float()
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    err = (y.float() - ref).abs().max().item()
    assert err <= 2 ** -8 * ref.abs().max().item() + 1e-3, err          # one bf16 rounding of the output
    # ... and against the unquantised fp32 product: what e4m3 costs (reported; SURVEY 8d asks cosine >= 0.999)
    full = x.float() @ w.float().t() + b.float() + r.float()
    cos = F.cosine_similarity(y.float().flatten(), full.flatten(), dim=0).item()
    assert cos > 0.999, cos


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 64, 64, 320, 320), (1, 32, 32, 640, 1280), (3, 17, 23, 128, 132),
                                            (16, 64, 64, 320, 320)])
def test_fp8_conv3x3_matches_fp32_of_the_dequantised_operands(N, H, W, Cin, Cout):
    from garmentdreamer_amd.nn_ops import fp8_conv3x3, fp8_pack_weights, fp8_quantize
    g = torch.Generator(DEV).manual_seed(H * W + Cin)
    x = torch.randn(N, Cin, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (9 * Cin) ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, Cout, device=DEV, generator=g).to(torch.bfloat16)      # per-image bias (time embedding)
    r = torch.randn(N, Cout, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    sx, sw = float(x.abs().max()) / 448.0, float(w.abs().max()) / 448.0
    x8 = fp8_quantize(x.permute(0, 2, 3, 1), sx).permute(0, 3, 1, 2)         # NHWC bytes viewed as [N, C, H, W]
    w8 = fp8_pack_weights(w.permute(0, 2, 3, 1).reshape(Cout * 9, Cin), sw)    # [Cout][3][3][Cin]
    y = fp8_conv3x3(x8, w8, b, r, Cin, sx * sw)
    _, xq = _e4m3(x.float() / sx)
    _, wq = _e4m3(w.float() / sw)
    ref = F.conv2d(xq, wq, padding=1) * (sx * sw) + b.float()[:, :, None, None] + r.float()
    assert y.shape == ref.shape and y.is_contiguous(memory_format=torch.channels_last)
    err = (y.float() - ref).abs().max().item()
    assert err <= 2 ** -8 * ref.abs().max().item() + 2e-3, err
    full = F.conv2d(x.float(), w.float(), padding=1) + b.float()[:, :, None, None] + r.float()
    assert F.cosine_similarity(y.float().flatten(), full.flatten(), dim=0).item() > 0.999


def test_fp8_gn_conv_site_matches_fp32_torch():
    """One fp8 site as the UNet runs it -- GroupNorm+SiLU -> e4m3 (one kernel), e4m3 3x3 convolution with per-image
    bias and residual -- against fp32 PyTorch (per-layer cosine >= 0.999)."""
    import torch.nn as nn
    from garmentdreamer_amd.nn_ops import Fp8State
    g = torch.Generator(DEV).manual_seed(11)
    N, C, Co, H = 4, 640, 320, 64
    x = (torch.randn(N, C, H, H, device=DEV, generator=g) * 1.7 + 0.3).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.device(DEV):
        norm, conv = nn.GroupNorm(32, C, eps=1e-5), nn.Conv2d(C, Co, 3, padding=1)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(C, device=DEV, generator=g) + 0.5); norm.bias.copy_(torch.randn(C, device=DEV, generator=g) * 0.2)
    norm, conv = norm.to(torch.bfloat16), conv.to(torch.bfloat16)
    bias = torch.randn(N, Co, device=DEV, generator=g).to(torch.bfloat16)
    res = torch.randn(N, Co, H, H, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        act = F.silu(F.group_norm(x.float(), 32, norm.weight.float(), norm.bias.float(), 1e-5))
        ref = F.conv2d(act, conv.weight.float(), padding=1) + bias.float()[:, :, None, None] + res.float()
        st = Fp8State()
        assert st.wants(conv, x)
        st.observe(conv, act)
        y = st.gn_conv(norm, conv, x, bias, res)
    cos = F.cosine_similarity(y.float().flatten(), ref.flatten(), dim=0).item()
    conv_only = (y.float() - bias.float()[:, :, None, None] - res.float())
    cos_conv = F.cosine_similarity(conv_only.flatten(), (ref - bias.float()[:, :, None, None] - res.float()).flatten(), dim=0).item()
    assert cos > 0.9995 and cos_conv > 0.999, (cos, cos_conv)


def test_fp8_unet_forward_close_to_bf16_and_fp32():
    """End to end: the UNet's no-grad forward with e4m3 convolutions (after one calibration call) against the same
    network in bf16 and in fp32 -- cosine of the noise prediction, reported in profiles/; reduced width."""
    from garmentdreamer_amd.guidance import sd21
    from tests import parity_report
    kw = dict(block_out_channels=(128, 256, 512, 512), attention_head_dim=(2, 4, 8, 8))
    with torch.device(DEV):
        unet = sd21.init_random_(sd21.UNet2DConditionModel(**kw))
    u32 = unet.float().eval()
    import copy
    u16 = copy.deepcopy(u32).to(torch.bfloat16).to(memory_format=torch.channels_last).eval()
    u8 = copy.deepcopy(u16)
    for m in (u32, u16, u8):
        for p in m.parameters():
            p.requires_grad_(False)
    st = u8.enable_fp8()
    g = torch.Generator(DEV).manual_seed(5)
    x = torch.randn(4, 4, 64, 64, device=DEV, generator=g)
    t = torch.tensor([37.0, 500.0, 731.0, 980.0], device=DEV)
    ctx = torch.randn(4, 77, 1024, device=DEV, generator=g)
    with torch.no_grad():
        e32 = u32(x, t, encoder_hidden_states=ctx)
        e16 = u16(x.to(torch.bfloat16), t, encoder_hidden_states=ctx.to(torch.bfloat16)).float()
        u8(x.to(torch.bfloat16), t, encoder_hidden_states=ctx.to(torch.bfloat16))          # calibration (bf16)
        assert st.mode == "calibrate" and len(st.amax) >= 16
        st.mode = "run"
        e8 = u8(x.to(torch.bfloat16), t, encoder_hidden_states=ctx.to(torch.bfloat16)).float()
    assert st.sites_run >= 16
    c16, c8, c8_16 = (F.cosine_similarity(a.flatten(), b.flatten(), dim=0).item() for a, b in ((e16, e32), (e8, e32), (e8, e16)))
    parity_report.record("fp8 UNet forward (reduced width) vs fp32", "eps", cos_bf16_vs_fp32=c16, cos_fp8_vs_fp32=c8,
                         cos_fp8_vs_bf16=c8_16, fp8_sites=st.sites_run)
    assert torch.isfinite(e8).all() and c8 > 0.99 and c8_16 > 0.99, (c16, c8, c8_16)


def test_conv3x3_tiny_cout_backward_stays_on_the_mfma_kernel():
    """The VAE's conv_out (512 -> 8): the input gradient runs on the own kernel with its K zero-padded to 64 (no MIOpen
    fallback) and matches fp32 PyTorch."""
    from garmentdreamer_amd.nn_ops import conv3x3
    g = torch.Generator(DEV).manual_seed(8)
    x = torch.randn(2, 512, 64, 64, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(8, 512, 3, 3, device=DEV, generator=g) / 68).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    b = torch.randn(8, device=DEV, generator=g).to(torch.bfloat16)
    xg = x.clone().requires_grad_(True)
    y = conv3x3(xg, w, b, None)
    gy = torch.randn(y.shape, device=DEV, generator=g).to(torch.bfloat16)
    y.backward(gy)
    xr = x.float().requires_grad_(True)
    yr = F.conv2d(xr, w.float(), b.float(), padding=1)
    yr.backward(gy.float())
    assert (y.float() - yr).abs().max().item() <= 2e-2 * yr.abs().max().item()
    assert F.cosine_similarity(xg.grad.float().flatten(), xr.grad.flatten(), dim=0).item() > 0.9995
    assert (xg.grad.float() - xr.grad).abs().max().item() <= 2e-2 * xr.grad.abs().max().item() + 1e-3


@pytest.mark.parametrize("B,H,S,Skv", [(2, 5, 4096, 77), (3, 20, 256, 77), (1, 10, 1024, 100), (2, 5, 300, 64), (2, 5, 320, 1)])
def test_attention_d64_with_a_key_count_that_is_not_a_multiple_of_64(B, H, S, Skv):
    """Cross-attention over the 77 text tokens (and other ragged key counts) on the own kernel: padded keys must get no
    weight.  K / V are column slices of a wider matrix (sd21.ContextProjections hands the kernel strided views)."""
    from garmentdreamer_amd.nn_ops import attention_d64, attention_d64_supported
    g = torch.Generator(DEV).manual_seed(S + Skv)
    q = (torch.randn(B, S, H * 64, device=DEV, generator=g) * 1.5).to(torch.bfloat16).view(B, S, H, 64)
    wide = (torch.randn(B, Skv, 3 * H * 64 + 128, device=DEV, generator=g) * 1.5).to(torch.bfloat16)
    k = wide[..., 64:64 + H * 64].view(B, Skv, H, 64)
    v = wide[..., 64 + H * 64:64 + 2 * H * 64].view(B, Skv, H, 64)
    assert attention_d64_supported(q, k, v)
    with torch.no_grad():
        out = attention_d64(q, k, v)
        ref = F.scaled_dot_product_attention(q.transpose(1, 2).float(), k.transpose(1, 2).float(), v.transpose(1, 2).float())
        ref = ref.transpose(1, 2).reshape(B, S, H * 64)
    assert torch.isfinite(out).all()
    err = (out.float() - ref).abs().max().item()
    assert err <= 2e-2 * ref.abs().max().item() + 2e-3, err
    assert F.cosine_similarity(out.float().flatten(), ref.flatten(), dim=0).item() > 0.9995


@pytest.mark.parametrize("B,H,S,Skv", [(2, 5, 4096, 77), (3, 20, 256, 77), (1, 10, 1024, 100), (2, 5, 320, 64)])
def test_cross_attention_with_v_transposed_as_a_strided_slice_is_the_same_kernel_result(B, H, S, Skv):
    """gd_nn_attention_d64_forward_vt_strided (round 5: the frozen UNet's cross-attention reads V^T of the text tokens as a
    channel slice of ONE all-layers W_v . context^T product, no transposing pre-pass): handed exactly the transpose of V --
    zero-padded to whole 64-key tiles, as a slice of a wider [B, sum C, Skv_pad] tensor -- it returns the bits of
    attention_d64 on the row-major V; and a wrong batch stride is refused."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(S * 3 + Skv)
    q = (torch.randn(B, S, H * 64, device=DEV, generator=g) * 1.5).to(torch.bfloat16).view(B, S, H, 64)
    wide = (torch.randn(B, Skv, 2 * H * 64 + 64, device=DEV, generator=g) * 1.5).to(torch.bfloat16)
    k = wide[..., 64:64 + H * 64].view(B, Skv, H, 64)
    v = (torch.randn(B, Skv, H * 64, device=DEV, generator=g) * 1.5).to(torch.bfloat16)
    Sp = (Skv + 63) // 64 * 64
    vt_all = torch.full((B, 3 * H * 64, Sp), float("nan"), dtype=torch.bfloat16, device=DEV)     # neighbours' slices: never read
    vt_all[:, H * 64:2 * H * 64, :Skv] = v.transpose(1, 2)
    vt_all[:, H * 64:2 * H * 64, Skv:] = 0
    vt = vt_all[:, H * 64:2 * H * 64]
    with torch.no_grad():
        ref = nn_ops.attention_d64(q, k, v.view(B, Skv, H, 64))
        out = nn_ops.attention_d64_vt_strided(q, k, vt, Skv)
    assert torch.isfinite(out).all() and torch.equal(out, ref)
    L = nn_ops.lib()
    o = torch.empty_like(out)
    bad = L.gd_nn_attention_d64_forward_vt_strided(torch.cuda.current_stream().cuda_stream, q.data_ptr(), k.data_ptr(), vt.data_ptr(),
                                                   o.data_ptr(), B, S, Sp, H, q.stride(0), q.stride(1), k.stride(0), k.stride(1),
                                                   H * 64 * Sp - 8, o.stride(0), o.stride(1), 0.125, Skv)
    assert bad < 0


def test_frozen_unet_cross_attention_reads_v_transposed_from_the_context_projection(monkeypatch):
    """sd21.UNet2DConditionModel._project_context: V^T of every cross-attention layer from one batched GEMM on the zero-padded
    context (ContextProjections.vt), consumed in place by the attention kernel -- against the same UNet with the per-layer
    row-major V + transposing pre-pass (GD_CTX_VT=0 behaviour): the two differ only in the summation order of the V GEMM."""
    from garmentdreamer_amd.guidance import sd21
    with torch.device(DEV):
        unet = sd21.init_random_(sd21.UNet2DConditionModel(block_out_channels=(64, 128, 256, 256), attention_head_dim=(1, 2, 4, 4)))
    unet = unet.to(torch.bfloat16).to(memory_format=torch.channels_last)
    for p in unet.parameters():
        p.requires_grad_(False)
    x = torch.randn(2, 4, 64, 64, device=DEV)
    t = torch.tensor([50, 800], device=DEV)
    c = torch.randn(2, 77, 1024, device=DEV)
    with torch.no_grad():
        proj = unet._project_context(c.to(torch.bfloat16))
        assert isinstance(proj, sd21.ContextProjections) and len(proj.vt) == len(proj.kv) > 0
        for key, (k_, v_) in proj.kv.items():          # the slices ARE the transposes (to GEMM rounding), padded keys zero
            vt = proj.vt[key]
            assert vt.shape == (2, v_.shape[-1], 128) and float(vt[..., 77:].abs().max()) == 0.0
            assert (vt[..., :77].transpose(1, 2).float() - v_.float()).abs().max().item() <= 2e-2 * v_.float().abs().max().item()
        y_on = unet(x, t, c).float()
        monkeypatch.setattr(sd21, "_CTX_VT", False)
        unet._ctx_cat = None
        y_off = unet(x, t, c).float()
    assert torch.isfinite(y_on).all()
    assert F.cosine_similarity(y_on.flatten(), y_off.flatten(), dim=0).item() > 0.9999
    assert (y_on - y_off).abs().max().item() <= 2e-2 * y_off.abs().max().item()


@pytest.mark.parametrize("M,N,with_bias", [(65536, 320, True), (4096, 320, True), (8192, 320, False), (65536 + 37, 320, True),
                                           (4096 + 1, 320, True), (32 * 256 * 5 + 31, 320, False), (65536, 640, False),
                                           (8192 + 5, 640, True), (65536, 2560, True), (4096 + 33, 2560, True)])
def test_linear_320_streaming_kernel_matches_fp32_reference(M, N, with_bias):
    """gd_nn_linear_320_forward (weights in registers, x streamed through four LDS stages by LDS-DMA, waits counted per
    instruction) against fp32 torch on the same bf16 operands: every element within one bf16 ulp of the fp32
    result (products of bf16 values are exact in fp32; sums of 320 of them in another order differ by ~1e-6 relative,
    which moves an occasional element across a rounding boundary: half an ulp is NOT a valid bound),
    ragged row counts, several tiles per workgroup and the 2- and 8-column-block forms (N = 640, 2560) included; two
    launches are bit-identical."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(M + N)
    x = torch.randn(M, 320, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, 320, device=DEV, generator=g) / 18).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g).to(torch.bfloat16) if with_bias else None
    assert nn_ops.linear_320_supported(x, w)
    y = nn_ops.linear_320(x, w, b)
    ref = F.linear(x.float(), w.float(), None if b is None else b.float())
    err = (y.float() - ref).abs()
    assert bool((err <= 2.0 ** -7 * ref.abs() + 1e-5).all()), float((err / (ref.abs() + 1e-3)).max())
    assert torch.equal(y, nn_ops.linear_320(x, w, b))
    # 3-D input as the transformer blocks pass it
    if M % 4096 == 0:
        y3 = nn_ops.linear_320(x.view(M // 4096, 4096, 320), w, b)
        assert y3.shape == (M // 4096, 4096, N) and torch.equal(y3.reshape(M, N), y)
    assert not nn_ops.linear_320_supported(x[:, :160], w[:, :160])       # other K: not this kernel's
    assert not nn_ops.linear_320_supported(x[:1024], w)                  # short row sets stay on the library


@pytest.mark.parametrize("M", [65536, 4096 + 33, 8192])
def test_linear_320_with_geglu_epilogue_is_bit_identical_to_the_two_kernels(M):
    """gd_nn_linear_k320_geglu_forward (GEGLU arithmetic in the streaming GEMM's store phase, on the bf16-rounded tile)
    against gd_nn_linear_k320_forward + gd_nn_geglu_forward: bit-identical; and against fp32 torch GEGLU."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(M)
    x = torch.randn(M, 320, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(2560, 320, device=DEV, generator=g) / 18).to(torch.bfloat16)
    b = torch.randn(2560, device=DEV, generator=g).to(torch.bfloat16)
    y = nn_ops.linear_320_geglu(x, w, b)
    two = nn_ops.geglu(nn_ops.linear_320(x, w, b))
    assert y.shape == (M, 1280) and torch.equal(y, two)
    h, gate = F.linear(x.float(), w.float(), b.float()).chunk(2, dim=-1)
    ref = h * F.gelu(gate)
    assert (y.float() - ref).abs().max().item() <= 2e-2 * ref.abs().max().item()


@pytest.mark.parametrize("M,K,N,res", [(4096, 320, 320, True), (1000, 640, 1920, False), (77, 1024, 640, False),
                                       (65536, 320, 2560, False), (513, 1280, 1284, True)])
def test_linear_one_tap_gemm_matches_fp32_reference(M, K, N, res):
    """gd_nn_linear_forward: nn.Linear (+ residual) as a one-tap launch of the implicit-GEMM convolution kernel
    (ragged M and N tiles, bias, residual).  An option, not the default path: hipBLASLt is faster on these shapes."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(M + K)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g).to(torch.bfloat16)
    r = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16) if res else None
    with torch.no_grad():
        assert nn_ops.linear_supported(x, w)
        y = nn_ops.linear(x, w, b, r).float()
    ref = x.float() @ w.float().t() + b.float() + (r.float() if res else 0.0)
    assert y.shape == ref.shape
    err = (y - ref).abs().max().item()
    assert err <= 1e-2 * ref.abs().max().item() + 1e-2, err
    assert F.cosine_similarity(y.flatten(), ref.flatten(), dim=0).item() > 0.9999


_WINO_WIDE_CASES = [  # N, Cin, Cout, H, W, per-image bias, residual, GroupNorm in the loader
    (1, 32, 64, 16, 16, False, False, False), (2, 64, 128, 48, 32, True, True, False), (3, 96, 72, 40, 56, False, True, False),
    (2, 128, 320, 64, 64, True, False, False), (1, 128, 128, 100, 36, False, False, False),
    (8, 128, 128, 128, 128, False, True, False), (2, 64, 128, 48, 32, True, True, True), (1, 32, 64, 16, 16, False, False, True),
    (2, 128, 128, 64, 80, False, True, True), (3, 320, 320, 32, 32, True, False, True), (2, 256, 256, 72, 40, False, False, True),
    (40, 64, 64, 32, 32, False, True, True)]


@pytest.mark.parametrize("N,Cin,Cout,H,W,per_image_bias,res,gn", _WINO_WIDE_CASES)
@pytest.mark.parametrize("kernel", ["wino", "wide"])
def test_winograd_and_wide_tile_convolutions_match_fp32_reference(kernel, N, Cin, Cout, H, W, per_image_bias, res, gn):
    """The two round-4 forms of the stride-1 3x3 convolution (csrc/nn_conv_wino.h: Winograd F(2,3) along x;
    csrc/nn_conv_wide.h: 128 channels x 16x32 pixels), plain and with GroupNorm+SiLU in the loader, through the C-ABI,
    against fp32 PyTorch: ragged sizes, Cout not a multiple of 128, one K chunk, per-image bias, residual, many tiles
    per CU -- and the GroupNorm partial sums of the epilogue against sums over the stored tensor.  Bar: the direct bf16
    kernels' (2e-2 of scale, cos > 0.9995); the Winograd form rounds its transformed inputs once more (measured 1.4x
    the direct kernels' error: 3.2-5.5e-3 of scale against 2.4-3.3e-3)."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(Cin * 7 + Cout + H)
    cl = torch.channels_last
    x = (torch.randn(N, Cin, H, W, device=DEV, generator=g) * 1.5 + 0.3).to(torch.bfloat16).contiguous(memory_format=cl)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (3 * Cin ** 0.5)).to(torch.bfloat16).contiguous(memory_format=cl)
    b = (torch.randn(N, Cout, device=DEV, generator=g) if per_image_bias else torch.randn(Cout, device=DEV, generator=g)).to(torch.bfloat16)
    r = torch.randn(N, Cout, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=cl) if res else None
    groups = 32
    rows = ((H + 15) // 16) * ((W + 15) // 16) * 8
    part = torch.full((N * (Cout // 4) * rows * 2,), float("nan"), dtype=torch.float32, device=DEV)   # every row must be written
    with torch.no_grad():
        xin = x.float()
        gnargs = None
        if gn:
            gw = (torch.randn(Cin, device=DEV, generator=g) * 0.5 + 1).to(torch.bfloat16)
            gb = (torch.randn(Cin, device=DEV, generator=g) * 0.5).to(torch.bfloat16)
            xin = F.silu(F.group_norm(xin, groups, gw.float(), gb.float(), 1e-6))
            xg = x.float().reshape(N, groups, -1)
            mr = torch.stack([xg.mean(-1), (xg.var(-1, unbiased=False) + 1e-6).rsqrt()], -1).reshape(-1).contiguous()
            gnargs = (mr, gw, gb, groups, True)
        ref = F.conv2d(xin, w.float(), None, padding=1)
        ref = ref + (b.float()[:, :, None, None] if per_image_bias else b.float()[None, :, None, None])
        if res:
            ref = ref + r.float()
        if kernel == "wide":
            y = nn_ops._wide_launch(x, w, b, r, Cout, part, gn=gnargs)
        elif gn:
            y = nn_ops._wino_gn_launch(x, mr, gw, gb, groups, True, w, b, r, Cout, part)
        else:
            y = nn_ops._wino_launch(x, w, b, r, Cout, part)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=cl)
    err = ((y.float() - ref).abs().max() / ref.abs().max()).item()
    cos = F.cosine_similarity(y.float().flatten(), ref.flatten(), dim=0).item()
    assert err < 2e-2 and cos > 0.9995, (err, cos)
    assert torch.isfinite(part).all()
    got = part.view(N, Cout // 4, rows, 2).double().sum(2)
    yq = y.float().double().view(N, Cout // 4, 4, H * W)
    want = torch.stack([yq.sum((2, 3)), (yq * yq).sum((2, 3))], -1)
    assert ((got - want).abs().max() / want.abs().max()).item() < 1e-5



@pytest.mark.parametrize("M,K,N,frozen", [(77 * 2, 1024, 320, None), (4096, 320, 320, None), (1000, 640, 640, "down"), (33, 1280, 1280, "up"),
                                          (8192, 320, 1280, None)])
def test_lora_branch_forward_and_backward_match_fp32_reference(M, K, N, frozen):
    """``base + scale * up(down(x))`` of the LoRA UNet's adapted projections (csrc/nn_lora.hip through the C-ABI): output and
    the four gradients (x, base, down, up) against fp32 PyTorch on the same bf16 inputs; bitwise reproducible."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(M + K)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16).requires_grad_(True)
    base = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16).requires_grad_(True)
    down = (torch.randn(4, K, device=DEV, generator=g) / 4).requires_grad_(True)
    up = (torch.randn(N, 4, device=DEV, generator=g) * 0.3).requires_grad_(True)
    dy = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    scale = 0.75
    if frozen:          # one frozen adapter half: the single-reduction path instead of the paired launch
        (down if frozen == "down" else up).requires_grad_(False)
    assert nn_ops.lora_branch_supported(x, base, down, up)
    outs = []
    for _ in range(2):
        for t in (x, base, down, up):
            t.grad = None
        y = nn_ops.lora_branch(x, base, down, up, scale)
        y.backward(dy)
        outs.append([y.detach().clone()] + [None if t.grad is None else t.grad.clone() for t in (x, base, down, up)])
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(*outs))
    xf, bf, df, uf = (t.detach().float().requires_grad_(True) for t in (x, base, down, up))
    yr = bf + scale * (xf @ df.t()) @ uf.t()
    yr.backward(dy.float())
    y, gx, gb, gd_, gu = outs[0]
    assert y.dtype == torch.bfloat16 and gx.dtype == torch.bfloat16
    assert (gd_ is None) == (frozen == "down") and (gu is None) == (frozen == "up")
    def rel(a, b):
        return ((a.float() - b).abs().max() / b.abs().max()).item()
    assert rel(y, yr.detach()) < 6e-3            # one bf16 rounding of the sum
    assert rel(gx, xf.grad) < 6e-3
    assert torch.equal(gb, dy)
    for got, want in ((gd_, df.grad), (gu, uf.grad)):       # fp32 sums over M in another order
        assert got is None or (got.dtype == torch.float32 and rel(got, want) < 2e-5)


@pytest.mark.parametrize("M,K,N", [(154, 1024, 320), (4096, 320, 320), (1001, 640, 1280), (33, 1280, 640)])
def test_lora_row_fused_is_bit_identical_to_rowdot_plus_rank4_add(M, K, N):
    """gd_nn_lora_row_fused (one wave computes a row's four dot products AND adds the rank-4 update) against the two
    launches it replaces, forward form (down, up, base) and backward form (up, down, optional base): the same bits in y
    and in the [M][4] intermediate."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(3 * M + K + N)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    base = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    down = torch.randn(4, K, device=DEV, generator=g) / 4
    up = torch.randn(N, 4, device=DEV, generator=g) * 0.3
    hs = nn_ops._lora_rowdot(x, down, 0.75, 0)
    want = nn_ops._lora_rank4_add(hs, up, base, N, 1)
    got, h = nn_ops._lora_row_fused(x, down, up, base, N, 0.75, 0)
    assert torch.equal(got, want) and torch.equal(h, hs)
    got2, h2 = nn_ops._lora_row_fused(x, down, up, base, N, 0.75, 0, want_h=False)
    assert h2 is None and torch.equal(got2, want)
    # backward form: a = dy [M][N], w1 = up [N][4], w2 = down [4][K]
    dy = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    dxb = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    dh = nn_ops._lora_rowdot(dy, up, 0.75, 1)
    for b in (None, dxb):
        want = nn_ops._lora_rank4_add(dh, down, b, K, 0)
        got, h = nn_ops._lora_row_fused(dy, up, down, b, K, 0.75, 1)
        assert torch.equal(got, want) and torch.equal(h, dh)


@pytest.mark.parametrize("shape,K,N,bias,x_grad", [((2, 2048, 320), 320, 320, False, True), ((2, 77, 1024), 1024, 640, False, False),
                                                   ((1, 1000, 640), 640, 640, True, True), ((3, 11, 1280), 1280, 1280, True, True)])
def test_lora_linear_node_matches_fp32_reference_and_the_two_node_path(shape, K, N, bias, x_grad):
    """nn_ops.lora_linear -- frozen projection + rank-4 adapter as ONE autograd node whose input gradient already holds both
    branches -- against fp32 PyTorch on the same bf16 inputs, and against F.linear + nn_ops.lora_branch (two nodes +
    autograd's add).  x without a gradient (the text tokens of the cross-attention's k / v) takes the no-dx path."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(K + N + shape[1])
    x = torch.randn(*shape, device=DEV, generator=g).to(torch.bfloat16).requires_grad_(x_grad)
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g).to(torch.bfloat16) if bias else None
    down = (torch.randn(4, K, device=DEV, generator=g) / 4).requires_grad_(True)
    up = (torch.randn(N, 4, device=DEV, generator=g) * 0.3).requires_grad_(True)
    dy = torch.randn(*shape[:-1], N, device=DEV, generator=g).to(torch.bfloat16)
    scale = 1.0
    res = {}
    for mode in ("node", "node", "two"):
        for t in (x, down, up):
            t.grad = None
        if mode == "node":
            y = nn_ops.lora_linear(x, w, down, up, scale, lambda t: F.linear(t, w, b))
        else:
            y = nn_ops.lora_branch(x, F.linear(x, w, b), down, up, scale)
        y.backward(dy)
        cur = [y.detach().clone(), None if x.grad is None else x.grad.clone(), down.grad.clone(), up.grad.clone()]
        if mode in res:          # bitwise reproducible
            assert all((p is None and q is None) or torch.equal(p, q) for p, q in zip(res[mode], cur))
        res[mode] = cur
    xf, wf, df, uf = x.detach().float().requires_grad_(x_grad), w.float(), down.detach().float().requires_grad_(True), up.detach().float().requires_grad_(True)
    yr = F.linear(xf, wf, None if b is None else b.float()) + scale * (xf @ df.t()) @ uf.t()
    yr.backward(dy.float())
    def rel(a, c):
        return ((a.float() - c).abs().max() / c.abs().max()).item()
    y, gx, gd_, gu = res["node"]
    assert y.shape == yr.shape and y.dtype == torch.bfloat16
    assert rel(y, yr.detach()) < 1.2e-2          # bf16 projection output + one bf16 rounding of the sum
    assert (gx is None) == (not x_grad)
    if x_grad:
        assert gx.shape == x.shape and rel(gx, xf.grad) < 1.2e-2
        # one rounding (fp32 sum of the two branches) where the two-node path rounds each branch and their sum
        assert rel(gx, xf.grad) <= rel(res["two"][1], xf.grad) * 1.5 + 1e-3
    assert rel(gd_, df.grad) < 2e-5 and rel(gu, uf.grad) < 2e-5
    assert torch.equal(y, res["two"][0]) and torch.equal(gd_, res["two"][2]) and torch.equal(gu, res["two"][3])


@pytest.mark.parametrize("B,H,W,bias", [(8, 64, 64, True), (1, 64, 64, True), (3, 17, 5, False)])
def test_quant_conv_1x1_forward_and_input_gradient_match_fp32_reference(B, H, W, bias):
    """gd_nn_conv1x1_c8 (AutoencoderKL.quant_conv, nn.Conv2d(8, 8, 1)) through the module the VAE holds: output and input
    gradient against fp32 F.conv2d on the same bf16 values; NCHW-contiguous input takes the layout conversion."""
    from garmentdreamer_amd.guidance import sd21
    g = torch.Generator(DEV).manual_seed(B + H)
    conv = sd21._QuantConv(8, 8, 1).to(DEV).to(torch.bfloat16).requires_grad_(False)
    with torch.no_grad():
        conv.weight.copy_((torch.randn(8, 8, 1, 1, device=DEV, generator=g) * 0.5).to(torch.bfloat16))
        if bias:
            conv.bias.copy_(torch.randn(8, device=DEV, generator=g).to(torch.bfloat16))
        else:
            conv.bias = None
    for fmt in (torch.channels_last, torch.contiguous_format):
        x = torch.randn(B, 8, H, W, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=fmt).requires_grad_(True)
        dy = torch.randn(B, 8, H, W, device=DEV, generator=g).to(torch.bfloat16)
        from garmentdreamer_amd import nn_ops
        assert nn_ops.conv1x1_c8_supported(x, conv.weight, conv.bias)
        y = conv(x)
        assert "Conv1x1C8" in type(y.grad_fn).__name__
        y.backward(dy)
        xf = x.detach().float().requires_grad_(True)
        yr = F.conv2d(xf, conv.weight.float(), None if conv.bias is None else conv.bias.float())
        yr.backward(dy.float())
        assert y.shape == yr.shape and x.grad.shape == x.shape
        assert (y.float() - yr).abs().max().item() <= 4e-3 * yr.abs().max().item() + 1e-6      # one bf16 rounding
        assert (x.grad.float() - xf.grad).abs().max().item() <= 4e-3 * xf.grad.abs().max().item() + 1e-6
    conv.weight.requires_grad_(True)          # a trainable quant_conv stays on F.conv2d
    assert not nn_ops.conv1x1_c8_supported(x, conv.weight, conv.bias)


@pytest.mark.parametrize("rows,L", [(300, 4096), (77, 1024), (5, 8192), (130, 264), (9, 8)])
def test_row_softmax_forward_and_backward_match_fp32_reference(rows, L):
    """gd_nn_softmax_rows_forward / _backward (the VAE mid block's attention scores), in place, against fp32 torch on the same
    bf16 values; rows of very different magnitude, a row of equal values and a masked-looking row included."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(rows + L)
    x = (torch.randn(rows, L, device=DEV, generator=g) * torch.logspace(-1, 1.3, rows, device=DEV)[:, None]).to(torch.bfloat16)
    x[0] = 3.0
    if L > 8:
        x[1, 1:] = -30000.0
    ref = torch.softmax(x.float(), -1)
    p = nn_ops.softmax_rows_(x.clone())
    assert p.dtype == torch.bfloat16 and torch.isfinite(p.float()).all()
    assert (p.float() - ref).abs().max().item() <= 4e-3 * ref.max().item() + 1e-6       # one bf16 rounding of a value <= 1
    assert (p.float().sum(-1) - 1).abs().max().item() < 2e-2
    dp = torch.randn(rows, L, device=DEV, generator=g).to(torch.bfloat16)
    pf = p.float().requires_grad_(True)
    want = torch._softmax_backward_data(dp.float(), pf.detach(), -1, torch.float32)
    got = nn_ops.softmax_rows_backward_(p, dp.clone())
    scale = want.abs().max().item()
    assert (got.float() - want).abs().max().item() <= 8e-3 * scale + 1e-7
    assert torch.equal(got, nn_ops.softmax_rows_backward_(p, dp.clone()))


def test_vae_mid_attention_node_matches_the_library_path_and_fp32():
    """sd21._VAEAttention with its core as one autograd node (library GEMMs on the packed projection, own in-place row softmax
    forward / backward, the three input gradients written into one tensor) against the chunk + torch.softmax path of the
    same module and against fp32: output and input gradient."""
    from garmentdreamer_amd.guidance import sd21
    g = torch.Generator(DEV).manual_seed(3)
    att = sd21._VAEAttention(512).to(DEV)
    sd21.init_random_(att, 4)
    ref32 = sd21._VAEAttention(512).to(DEV)
    ref32.load_state_dict(att.state_dict())
    att = att.to(torch.bfloat16).requires_grad_(False)
    x = torch.randn(2, 512, 32, 32, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(2, 512, 32, 32, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    res = {}
    for node in (True, False):
        sd21._VAE_ATTN_NODE = node
        try:
            xi = x.detach().clone().requires_grad_(True)
            y = att(xi)
            y.backward(gy)
            res[node] = (y.detach().float(), xi.grad.float())
        finally:
            sd21._VAE_ATTN_NODE = True
    ref32 = ref32.requires_grad_(False)
    w = {k: v.to(torch.bfloat16).float() for k, v in ref32.state_dict().items()}
    ref32.load_state_dict(w)
    xr = x.detach().float().contiguous().requires_grad_(True)
    hh = F.group_norm(xr, 32, ref32.group_norm.weight, ref32.group_norm.bias, 1e-6).permute(0, 2, 3, 1).reshape(2, 1024, 512)
    q, k, v = ref32.to_q(hh), ref32.to_k(hh), ref32.to_v(hh)
    o = torch.softmax(q @ k.transpose(1, 2) * 512 ** -0.5, -1) @ v
    yr = xr + ref32.to_out[0](o).reshape(2, 32, 32, 512).permute(0, 3, 1, 2)
    yr.backward(gy.float())
    def rel(a, b):
        return ((a - b).abs().max() / b.abs().max()).item()
    (y1, g1), (y0, g0) = res[True], res[False]
    assert rel(y1, yr.detach()) < 2e-2 and rel(g1, xr.grad) < 3e-2
    assert rel(y1, y0) < 1e-2 and rel(g1, g0) < 1.5e-2
    assert F.cosine_similarity(g1.flatten(), xr.grad.flatten(), dim=0).item() > 0.9995
    assert rel(g1, xr.grad) <= 1.3 * rel(g0, xr.grad) + 2e-3


def test_lora_gradients_land_in_the_flat_adam_sinks():
    """With flat_adam.FlatAdam the adapters' .grad are slices of one flat buffer and the LoRA backward kernels add into them
    (gd_nn_lora_colreduce_pair_into): the same bits as the gradients the node returns without sinks, twice that after a
    second backward pass (accumulation), nothing handed to autograd; the update equals torch.optim.Adam's on those gradients."""
    from garmentdreamer_amd import nn_ops
    from garmentdreamer_amd.flat_adam import FlatAdam
    g = torch.Generator(DEV).manual_seed(5)
    M, K, N = 2048, 320, 640
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16).requires_grad_(True)
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).to(torch.bfloat16)
    dy = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    down0, up0 = torch.randn(4, K, device=DEV, generator=g) / 4, torch.randn(N, 4, device=DEV, generator=g) * 0.3
    def run(down, up, node):
        if node:
            y = nn_ops.lora_linear(x, w, down, up, 0.5, lambda t: F.linear(t, w))
        else:
            y = nn_ops.lora_branch(x, F.linear(x, w), down, up, 0.5)
        x.grad = None
        y.backward(dy)
        return y.detach(), x.grad.clone()
    for node in (True, False):
        down_r, up_r = torch.nn.Parameter(down0.clone()), torch.nn.Parameter(up0.clone())
        y_r, gx_r = run(down_r, up_r, node)
        down, up = torch.nn.Parameter(down0.clone()), torch.nn.Parameter(up0.clone())
        opt = FlatAdam([down, up], lr=1e-2, flat=[down, up])
        y, gx = run(down, up, node)
        assert torch.equal(y, y_r) and torch.equal(gx, gx_r)
        assert down.grad is down._gd_grad_sink and up.grad is up._gd_grad_sink
        assert torch.equal(down.grad, down_r.grad) and torch.equal(up.grad, up_r.grad)
        run(down, up, node)
        assert torch.equal(down.grad, 2 * down_r.grad) and torch.equal(up.grad, 2 * up_r.grad)
        opt.zero_grad()
        assert float(down.grad.abs().sum()) == 0.0 and float(up.grad.abs().sum()) == 0.0
        run(down, up, node)
        ropt = torch.optim.Adam([down_r, up_r], lr=1e-2)
        opt.step()
        ropt.step()
        assert torch.allclose(down.detach(), down_r.detach(), rtol=2e-6, atol=2e-7)
        assert torch.allclose(up.detach(), up_r.detach(), rtol=2e-6, atol=2e-7)


def test_grouped_lora_weight_gradients_are_the_per_adapter_launches_bit_for_bit():
    """nn_ops.lora_grad_group (round 6): the adapted projections created inside record their weight-gradient problems in their
    backward and the LAST one launches them all, 32 per launch with the table in the kernel arguments.  A chain of 70 adapted
    projections of four different shapes (three launches per stage), gradients into FlatAdam's sinks: the same bits as one
    gd_nn_lora_colreduce_pair_into per adapter, twice that after a second pass (accumulation), nothing pending at the end --
    and FlatAdam.step refuses to step over a group whose backward never reached all of its projections."""
    from garmentdreamer_amd import nn_ops
    from garmentdreamer_amd.flat_adam import FlatAdam
    g = torch.Generator(DEV).manual_seed(9)
    shapes = [(1024, 320, 320), (1024, 320, 640), (256, 640, 640), (64, 1280, 1280)]
    layers = []
    for i in range(70):
        M, K, N = shapes[i % 4]
        w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).to(torch.bfloat16)
        down = torch.nn.Parameter(torch.randn(4, K, device=DEV, generator=g) / 4)
        up = torch.nn.Parameter(torch.randn(N, 4, device=DEV, generator=g) * 0.3)
        x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16).requires_grad_(True)
        dy = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
        layers.append((x, w, down, up, dy))
    params = [p for _, _, d, u, _ in layers for p in (d, u)]
    opt = FlatAdam(params, lr=1e-3, flat=params)

    def run(grouped):
        opt.zero_grad()
        ctx = nn_ops.lora_grad_group() if grouped else __import__("contextlib").nullcontext()
        with ctx as grp:
            ys = [nn_ops.lora_linear(x, w, d, u, 0.5, (lambda t, w=w: F.linear(t, w))) for x, w, d, u, _ in layers]
        torch.autograd.backward(ys, [dy for *_, dy in layers])
        torch.cuda.synchronize()
        return [p.grad.clone() for p in params], grp

    ref, _ = run(False)
    got, grp = run(True)
    assert grp is not None and grp.expected == 70 and grp.launches == 1 and nn_ops.lora_groups_pending() == 0
    assert all(float(r.abs().max()) > 0 for r in ref)
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    # accumulation across two grouped passes without zero_grad
    with nn_ops.lora_grad_group():
        ys = [nn_ops.lora_linear(x, w, d, u, 0.5, (lambda t, w=w: F.linear(t, w))) for x, w, d, u, _ in layers]
    torch.autograd.backward(ys, [dy for *_, dy in layers])
    for a, p in zip(ref, params):
        assert torch.equal(p.grad, 2 * a)
    # a backward pass that misses one projection leaves its group open: the optimizer says so instead of stepping
    opt.zero_grad()
    with nn_ops.lora_grad_group():
        ys = [nn_ops.lora_linear(x, w, d, u, 0.5, (lambda t, w=w: F.linear(t, w))) for x, w, d, u, _ in layers]
    torch.autograd.backward(ys[:-1], [dy for *_, dy in layers][:-1])
    assert nn_ops.lora_groups_pending() == 69
    with pytest.raises(RuntimeError, match="never launched"):
        opt.step()
    del ys
    import gc
    gc.collect()


@pytest.mark.parametrize("rows,C", [(4096, 320), (1024, 640), (300, 1280), (77, 1024)])
def test_training_row_passes_forward_and_backward_match_fp32_reference(rows, C):
    """GEGLU and add + LayerNorm with a gradient on the activations (the LoRA UNet's training pass; frozen norm parameters):
    own forward kernels under autograd nodes whose backward is ONE kernel each (gd_nn_geglu_backward,
    gd_nn_layernorm_backward) against fp32 PyTorch on the same bf16 inputs."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(rows + C)
    def rel(a, b):
        return ((a.float() - b).abs().max() / b.abs().max()).item()
    # GEGLU
    x = (torch.randn(2, rows // 2 if rows % 2 == 0 else rows, 2 * C, device=DEV, generator=g) * 1.3).to(torch.bfloat16).requires_grad_(True)
    dy = torch.randn(*x.shape[:-1], C, device=DEV, generator=g).to(torch.bfloat16)
    y = nn_ops.geglu(x)
    assert y.grad_fn is not None and "Geglu" in type(y.grad_fn).__name__
    y.backward(dy)
    xf = x.detach().float().requires_grad_(True)
    h, gate = xf.chunk(2, -1)
    yr = h * F.gelu(gate)
    yr.backward(dy.float())
    assert rel(y.detach(), yr.detach()) < 1.2e-2 and rel(x.grad, xf.grad) < 1.2e-2
    # add + LayerNorm, with and without a residual; s is used downstream too (the residual stream)
    norm = torch.nn.LayerNorm(C, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        norm.weight.copy_((torch.randn(C, device=DEV, generator=g) * 0.3 + 1).to(torch.bfloat16))
        norm.bias.copy_((torch.randn(C, device=DEV, generator=g) * 0.3).to(torch.bfloat16))
    norm.requires_grad_(False)
    for with_res in (True, False):
        a = (torch.randn(rows, C, device=DEV, generator=g) * 2 + 0.5).to(torch.bfloat16).requires_grad_(True)
        r = torch.randn(rows, C, device=DEV, generator=g).to(torch.bfloat16).requires_grad_(True) if with_res else None
        gy = torch.randn(rows, C, device=DEV, generator=g).to(torch.bfloat16)
        gs = torch.randn(rows, C, device=DEV, generator=g).to(torch.bfloat16)
        s_, y_ = nn_ops.add_layer_norm(a, r, norm)
        assert "AddLayerNormTrain" in type(y_.grad_fn).__name__
        (y_.float() * gy.float()).sum().add((s_.float() * gs.float()).sum()).backward()
        af = a.detach().float().requires_grad_(True)
        rf = r.detach().float().requires_grad_(True) if with_res else None
        sf = (af + rf).to(torch.bfloat16).float() if with_res else af      # the residual stream is rounded to bf16, as in eager
        sf_graph = af + rf if with_res else af
        yf = F.layer_norm(sf_graph, (C,), norm.weight.float(), norm.bias.float(), norm.eps)
        ((yf * gy.float()).sum() + (sf_graph * gs.float()).sum()).backward()
        assert rel(y_.detach(), yf.detach()) < 2.5e-2, rel(y_.detach(), yf.detach())
        assert rel(a.grad, af.grad) < 1.5e-2, rel(a.grad, af.grad)
        if with_res:
            assert torch.equal(a.grad, r.grad)


@pytest.mark.parametrize("B,S,Skv,H", [(2, 256, 256, 5), (1, 1024, 77, 10), (2, 4096, 4096, 5), (1, 320, 320, 20), (1, 4096, 77, 5),
                                       (2, 256, 77, 20), (1, 1024, 200, 10), (1, 128, 77, 5)])
def test_attention_training_node_matches_fp32_reference(B, S, Skv, H):
    """The own forward kernel with its log-sum-exp output + the library's flash backward (nn_ops.attention_d64_train: the LoRA
    UNet's training pass) against fp32 PyTorch: output, the LSE tensor itself, and dq / dk / dv; self- and cross-attention
    shapes, strided [B, S, H, 64] views of wider projections."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(S + Skv + H)
    C = H * 64
    wq = (torch.randn(B, S, C + 64, device=DEV, generator=g)).to(torch.bfloat16)
    wkv = (torch.randn(B, Skv, 2 * C, device=DEV, generator=g)).to(torch.bfloat16)
    q = wq[..., :C].view(B, S, H, 64).detach().requires_grad_(True)
    k = wkv[..., :C].view(B, Skv, H, 64).detach().requires_grad_(True)
    v = wkv[..., C:].view(B, Skv, H, 64).detach().requires_grad_(True)
    assert nn_ops.attention_d64_train_supported(q, k, v)
    do = torch.randn(B, S, C, device=DEV, generator=g).to(torch.bfloat16)
    o = nn_ops.attention_d64_train(q, k, v)
    lse = o.grad_fn.saved_tensors[4].clone()
    grads = {}
    try:
        for own in (True, False):       # own backward kernels (self-attention) / the library's flash backward on the own LSE
            nn_ops._ATTN_BWD = own
            grads[own] = torch.autograd.grad(o, (q, k, v), do, retain_graph=True)
    finally:
        nn_ops._ATTN_BWD = True
    qf, kf, vf = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    sc = torch.einsum("bshd,bthd->bhst", qf, kf) / 8.0
    of = torch.einsum("bhst,bthd->bshd", torch.softmax(sc, -1), vf).reshape(B, S, C)
    of.backward(do.float())
    assert (lse - torch.logsumexp(sc.detach(), -1)).abs().max().item() < 2e-3
    def rel(a, b):
        return ((a.float() - b).abs().max() / b.abs().max()).item()
    assert rel(o.detach(), of.detach()) < 2e-2
    for own in (True, False):
        gq, gk, gv = grads[own]
        assert rel(gq, qf.grad) < 2e-2 and rel(gk, kf.grad) < 2e-2 and rel(gv, vf.grad) < 2e-2, own
    # the two backward paths are different code: never bit-identical.  Round 5: the own kernels serve EVERY key count (the
    # key-owning kernel deals the query tiles of a one-key-block head -- the 77 text tokens -- to several workgroups and
    # attn_bwd_reduce_kernel adds their fp32 partials); the round-4 routing (library below 256 keys) stays reachable
    assert not any(torch.equal(a, b) for a, b in zip(grads[True], grads[False]))
    if Skv < 256:
        try:
            nn_ops._ATTN_BWD_MIN_KEYS = 256
            lib_grads = torch.autograd.grad(o, (q, k, v), do, retain_graph=True)
        finally:
            nn_ops._ATTN_BWD_MIN_KEYS = 1
        assert all(torch.equal(a, b) for a, b in zip(lib_grads, grads[False]))
        again = torch.autograd.grad(o, (q, k, v), do, retain_graph=True)        # chunked reduction: bitwise reproducible
        assert all(torch.equal(a, b) for a, b in zip(again, grads[True]))


def test_conv_routing_picks_the_measured_kernel_and_all_routes_agree():
    """nn_ops._conv_route (the per-shape table of tools/wino_route_bench.py) and the three kernels behind it give the
    same convolution: direct (GD_NN_WINO=0 behaviour), Winograd, wide tile on one shape each route serves."""
    from garmentdreamer_amd import nn_ops
    assert nn_ops._conv_route(8, 512, 512, 128, 128) == "wide"
    assert nn_ops._conv_route(8, 512, 512, 128, 128, gn=True) == "wide"
    assert nn_ops._conv_route(8, 128, 128, 512, 512) == "wino"
    assert nn_ops._conv_route(16, 32, 32, 1280, 640) == "wide" and nn_ops._conv_route(8, 32, 32, 1280, 640) == "wino"
    assert nn_ops._conv_route(16, 64, 64, 320, 320) == "wino"
    assert nn_ops._conv_route(8, 256, 256, 256, 256) is None and nn_ops._conv_route(8, 256, 256, 256, 256, gn=True) is None
    assert nn_ops._conv_route(2, 16, 16, 1280, 1280) is None          # too few tiles: split-K implicit GEMM
    g = torch.Generator(DEV).manual_seed(5)
    cl = torch.channels_last
    x = torch.randn(16, 320, 64, 64, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=cl)
    w = (torch.randn(128, 320, 3, 3, device=DEV, generator=g) / 50).to(torch.bfloat16).contiguous(memory_format=cl)
    with torch.no_grad():
        ref = F.conv2d(x.float(), w.float(), None, padding=1)
        ys = [nn_ops._patch_launch(x, w, None, None, 128), nn_ops._wino_launch(x, w, None, None, 128),
              nn_ops._wide_launch(x, w, None, None, 128), nn_ops._conv_launch(x, w, None, None, 128)]
    for y in ys:
        assert ((y.float() - ref).abs().max() / ref.abs().max()).item() < 1e-2
    assert torch.equal(ys[1], ys[3])         # 128 wide tiles are too few: the router sent this shape to the Winograd kernel


def test_conv_profile_counts_one_record_with_the_algorithmic_flops_and_bytes_per_entry_call():
    """The event profile behind bench.py's roofline line: every entry call of the convolution family is ONE record of
    2 * M * Cout * taps * Cin flops and 2 * (input elements + taps * Cin * Cout + M * Cout [+ M * Cout with a residual]) bytes
    -- a split-K launch with its reduce is one record, the four parity classes of the upsample-fused convolution are one
    record whose input counts once.  Integers held in doubles: compared for equality.  Each case once without and once with
    a residual, but the upsample-fused entry, which takes none."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(11)
    cl = torch.channels_last

    def act(*shape):
        return torch.randn(*shape, device=DEV, generator=g).to(torch.bfloat16).contiguous(memory_format=cl)

    def filt(co, ci):
        return (torch.randn(co, ci, 3, 3, device=DEV, generator=g) / 30).to(torch.bfloat16).contiguous(memory_format=cl)

    def conv_case(call, N, Cin, Cout, H, W):      # nine taps, stride 1
        x, w = act(N, Cin, H, W), filt(Cout, Cin)
        M = N * H * W
        return [(lambda r=r: call(x, w, None, r, Cout), 2 * M * Cout * 9 * Cin,
                 2 * (M * Cin + 9 * Cin * Cout + M * Cout + (M * Cout if r is not None else 0)))
                for r in (None, act(N, Cout, H, W))]

    def forced_split(x, w, b, r, co):
        nn_ops.lib().gd_nn_conv_force_split(2)
        try:
            return nn_ops._conv_launch(x, w, b, r, co)
        finally:
            nn_ops.lib().gd_nn_conv_force_split(-1)

    cases = conv_case(nn_ops._conv_launch, 1, 64, 64, 8, 8)            # implicit GEMM, unsplit
    cases += conv_case(forced_split, 1, 128, 64, 8, 8)                 # split-K + reduce
    cases += conv_case(nn_ops._patch_launch, 1, 64, 64, 16, 16)
    cases += conv_case(nn_ops._wino_launch, 1, 32, 64, 16, 32)
    cases += conv_case(nn_ops._wide_launch, 1, 32, 64, 16, 32)
    xu, wu = act(1, 64, 8, 8), filt(64, 64)                            # four classes of 64 pixels, four taps each
    cases.append((lambda: nn_ops.upsample2x_conv3x3(xu, wu), 4 * 2 * 64 * 64 * 4 * 64,
                  2 * (64 * 64 + 4 * (4 * 64 * 64 + 64 * 64))))
    xl = torch.randn(128, 64, device=DEV, generator=g).to(torch.bfloat16)
    wl = (torch.randn(64, 64, device=DEV, generator=g) / 8).to(torch.bfloat16)
    for r in (None, torch.randn(128, 64, device=DEV, generator=g).to(torch.bfloat16)):     # one tap
        cases.append((lambda r=r: nn_ops.linear(xl, wl, None, r), 2 * 128 * 64 * 64,
                      2 * (128 * 64 + 64 * 64 + 128 * 64 + (128 * 64 if r is not None else 0))))
    assert nn_ops.lib().gd_nn_conv3x3_ws_bytes(1, 8, 8, 64, 64) == 0          # the first case is indeed unsplit
    nn_ops.conv_profile(enable=True, reset=True)
    try:
        with torch.no_grad():
            for call, flops, nbytes in cases:
                _, n0, f0 = nn_ops.conv_profile()
                b0 = nn_ops.conv_profile_bytes()
                call()
                _, n1, f1 = nn_ops.conv_profile()
                assert n1 - n0 == 1
                assert f1 - f0 == flops
                assert nn_ops.conv_profile_bytes() - b0 == nbytes
    finally:
        nn_ops.conv_profile(enable=False, reset=True)


_STEP_CONV_SHAPES = [   # (N, Cin, Cout, H): every stride-1 3x3 shape of the 8-view step that leaves the direct kernels (profiles/r04_conv_shapes.txt)
    (8, 128, 128, 512), (8, 256, 128, 256), (8, 512, 256, 128), (8, 512, 512, 128), (8, 512, 512, 64),
    (16, 320, 320, 64), (16, 640, 320, 64), (16, 960, 320, 64), (16, 640, 640, 64), (16, 320, 640, 32), (16, 640, 640, 32),
    (16, 1920, 640, 32), (16, 1280, 640, 32), (16, 960, 640, 32), (16, 1280, 1280, 32), (16, 640, 1280, 16), (16, 1280, 1280, 16),
    (16, 2560, 1280, 16), (16, 1920, 1280, 16)]


@pytest.mark.parametrize("N,Cin,Cout,H", _STEP_CONV_SHAPES)
def test_every_routed_shape_of_the_step_holds_the_stated_error_bound_against_fp32(N, Cin, Cout, H):
    """The round-4 advisor's Winograd item: the F(2,3) kernel rounds the TRANSFORMED inputs and filters to bf16 (a second rounding
    the direct kernels do not have), and a layer's forward pass may run on it while its gradient runs elsewhere.  Stated bound,
    asserted for every shape of the 8-view step that `nn_ops._conv_route` sends to the Winograd or the wide-tile kernel, AT the
    step's batch and map size, against fp32 convolution of the same bf16 operands: max error <= 6e-3 of the output scale,
    relative rms <= 3.2e-3, cosine > 0.99999 (measured on all 19 shapes: Winograd rms 2.57-2.66e-3, max 3.0-3.8e-3; wide tile rms
    1.66e-3 -- the bf16 rounding of the output alone --, max 1.9-2.3e-3; profiles/r05_parity_report.json).  Unit-variance
    activations with a mean (GroupNorm+SiLU outputs are not centred), filters of the networks' scale."""
    from garmentdreamer_amd import nn_ops
    from tests import parity_report
    route = nn_ops._conv_route(N, H, H, Cin, Cout)
    assert route in ("wino", "wide"), route
    g = torch.Generator(DEV).manual_seed(Cin + Cout + H)
    cl = torch.channels_last
    x = (torch.randn(N, Cin, H, H, device=DEV, generator=g) + 0.3).to(torch.bfloat16).contiguous(memory_format=cl)
    w = (torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (3 * Cin ** 0.5)).to(torch.bfloat16).contiguous(memory_format=cl)
    b = torch.randn(Cout, device=DEV, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        y = nn_ops._conv_launch(x, w, b, None, Cout).float()
        # fp32 reference image by image (the 512^2 activations are 1 GB in fp32)
        ref = torch.cat([F.conv2d(x[i:i + 1].float(), w.float(), b.float(), padding=1) for i in range(N)])
    scale = ref.abs().max().item()
    err = (y - ref).abs().max().item() / scale
    rms = ((y - ref).square().mean().sqrt() / ref.square().mean().sqrt()).item()
    cos = F.cosine_similarity(y.flatten(), ref.flatten(), dim=0).item()
    parity_report.record(f"conv3x3 {route} route, N{N} {Cin}->{Cout} @{H}^2 vs fp32", "kernel", max_err_of_scale=err, rel_rms=rms, cos=cos)
    assert err <= 6e-3 and rms <= 3.2e-3 and cos > 0.99999, (route, err, rms, cos)


def test_linear_320_counted_waits_under_competing_traffic():
    """The streaming K = 320 GEMM waits with ``s_waitcnt vmcnt(n)``, n counted per instruction (csrc/nn_linear.hip): a tile
    consumed before its LDS-DMA landed would be off by O(1).  Many launches on fresh data, alone and with a second stream
    keeping HBM busy, every element checked (the suite-resident form of tools/linear320_stress.py)."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(0)
    side = torch.cuda.Stream()
    big = torch.randn(32 * 1024 * 1024, device=DEV)
    for it in range(48):
        M = [65536, 16384, 4096 + 32 * (it % 7) + (it % 3), 32768][it % 4]
        N = [320, 640, 2560][it % 3]
        x = torch.randn(M, 320, device=DEV, generator=g).to(torch.bfloat16)
        w = (torch.randn(N, 320, device=DEV, generator=g) / 18).to(torch.bfloat16)
        b = torch.randn(N, device=DEV, generator=g).to(torch.bfloat16)
        if it % 2:
            with torch.cuda.stream(side):
                for _ in range(4):
                    big.mul_(1.0001)
        y = nn_ops.linear_320(x, w, b)
        ref = F.linear(x.float(), w.float(), b.float())
        assert bool(((y.float() - ref).abs() <= 2.0 ** -7 * ref.abs() + 1e-5).all()), (it, M, N)
        if N == 2560:
            assert torch.equal(nn_ops.linear_320_geglu(x, w, b), nn_ops.geglu(y))
    torch.cuda.synchronize()


def test_linear_320_dispatch_refuses_misaligned_views():
    from garmentdreamer_amd import nn_ops
    x = torch.randn(4096, 320, device=DEV).to(torch.bfloat16)
    w = torch.randn(320, 320, device=DEV).to(torch.bfloat16)
    b = torch.randn(324, device=DEV).to(torch.bfloat16)
    assert nn_ops.linear_320_supported(x, w, b[:320])
    assert not nn_ops.linear_320_supported(x, w, b[1:321])                          # bias at an odd element offset
    assert not nn_ops.linear_320_supported(x, w, b[:320].float())                   # fp32 bias
    wbuf = torch.randn(320 * 320 + 8, device=DEV).to(torch.bfloat16)
    assert not nn_ops.linear_320_supported(x, wbuf[1:1 + 320 * 320].view(320, 320))  # weight 2 bytes off a 16-byte boundary


# ---- the own GEMM (csrc/nn_gemm.hip): persistent 256 x 256 x 64 tiles, ten-slot LDS-DMA ring, fused epilogues -------------------
@pytest.mark.parametrize("M,K,N", [(256, 64, 256), (4096, 1280, 1280), (1000, 640, 648), (16384, 640, 5120), (77, 1024, 320),
                                   (513, 320, 264), (65536, 1280, 320), (300, 5120, 1280)])
def test_own_gemm_matches_fp32_with_bias_and_residual(M, K, N):
    """y = x W^T + b (+ residual) against fp32 PyTorch: full tiles, ragged rows and channels (zero fill by the buffer range check,
    masked stores), one K tile and eighty, a single workgroup and several passes of the persistent grid; rtol of bf16 outputs."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g).to(torch.bfloat16)
    r = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    assert nn_ops.gemm_supported(x, w, b, r)
    ref = F.linear(x.float(), w.float(), b.float())
    scale = ref.abs().max().item()
    for bias in (None, b):
        y = nn_ops.gemm(x, w, bias)
        want = ref if bias is not None else ref - b.float()
        assert (y.float() - want).abs().max().item() <= 8e-3 * scale, (M, K, N, bias is not None)
    # residual: the accumulators start as residual + bias -- ONE rounding, like torch.addmm (not the eager pair's two)
    y = nn_ops.gemm(x, w, b, r)
    assert (y.float() - (ref + r.float())).abs().max().item() <= 8e-3 * (ref + r.float()).abs().max().item()
    assert torch.equal(nn_ops.gemm(x, w, None, torch.zeros_like(r)), nn_ops.gemm(x, w))
    # batch invariance by construction: a row's bits do not depend on which other rows are in the call
    if M >= 512:
        part = nn_ops.gemm(x[M // 2 - 100:M // 2 + 157].contiguous(), w, b)
        assert torch.equal(part, nn_ops.gemm(x, w, b)[M // 2 - 100:M // 2 + 157])


@pytest.mark.parametrize("M,K,inner", [(256, 64, 128), (4096, 1280, 5120), (16384, 640, 2560), (1000, 320, 1288), (130, 1280, 5120)])
def test_own_gemm_geglu_epilogue_is_the_projection_followed_by_the_geglu_kernel(M, K, inner):
    """diffusers GEGLU(K, inner) as ONE kernel: bit-identical to the own GEMM followed by gd_nn_geglu_forward (same rounding
    points), and within bf16 tolerance of the fp32 composition."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(device=DEV).manual_seed(M + inner)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(2 * inner, K, device=DEV, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(2 * inner, device=DEV, generator=g).to(torch.bfloat16)
    assert nn_ops.gemm_supported(x, w, b, geglu=True)
    for bias in (b, None):
        y = nn_ops.gemm_geglu(x, w, bias)
        two = nn_ops.geglu(nn_ops.gemm(x, w, bias))
        assert torch.equal(y, two)
        h, gate = F.linear(x.float(), w.float(), None if bias is None else bias.float()).chunk(2, -1)
        ref = h * F.gelu(gate)
        assert (y.float() - ref).abs().max().item() <= 1.2e-2 * ref.abs().max().item()


def test_own_gemm_repeated_calls_are_bitwise_reproducible_and_refuses_what_it_cannot_do():
    from garmentdreamer_amd import nn_ops
    x = torch.randn(5000, 640, device=DEV).to(torch.bfloat16)
    w = torch.randn(1280, 640, device=DEV).to(torch.bfloat16)
    a = nn_ops.gemm(x, w)
    for _ in range(3):
        assert torch.equal(a, nn_ops.gemm(x, w))
    assert not nn_ops.gemm_supported(x[:, :100].contiguous(), w[:, :100].contiguous())      # K % 64
    with pytest.raises(RuntimeError, match="gd_nn_gemm_forward"):
        nn_ops.gemm(x[:, :96].contiguous(), w[:, :96].contiguous())
