"""The launch path of nn_ops on the GPU: the stream a kernel runs on is the current one, and a refused call raises with the
entry's name and its own text."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_launch_takes_the_current_stream_and_names_the_refused_entry():
    """GroupNorm on the default stream and inside ``torch.cuda.stream(s)``: equal bits, and one statistics workspace per
    stream.  On this shape ``group_norm_silu`` takes the one-launch form, which has no workspace, so the two-pass form
    behind it (``_GroupNormSiLU``, keyed by stream in ``_gn_workspace``) runs next to it on both streams."""
    from garmentdreamer_amd import nn_ops
    g = torch.Generator(DEV).manual_seed(11)
    x = (torch.randn(2, 32, 8, 8, device=DEV, generator=g) * 1.7 + 0.4).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    w = (torch.randn(32, device=DEV, generator=g) * 0.5 + 1.0).to(torch.bfloat16)
    b = (torch.randn(32, device=DEV, generator=g) * 0.3).to(torch.bfloat16)
    tag = "test_nn_launch_gpu"          # a workspace tag of this test's own: its cache entries are new, whatever ran before
    assert not [k for k in nn_ops._gn_ws_cache if k[2] == tag]

    def both():
        with torch.no_grad(), nn_ops.workspace_tag(tag):
            return nn_ops.group_norm_silu(x, w, b, 8, 1e-5, True), nn_ops._GroupNormSiLU.apply(x, w, b, 8, 1e-5, True)

    main = torch.cuda.current_stream(DEV)
    y0, z0 = both()
    s = torch.cuda.Stream(DEV)
    assert s.cuda_stream != main.cuda_stream
    s.wait_stream(main)
    with torch.cuda.stream(s):
        y1, z1 = both()
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(z0, z1)
    assert torch.isfinite(z0.float()).all() and z0.float().abs().max().item() > 0.5
    keys = {(0, main.cuda_stream, tag), (0, s.cuda_stream, tag)}
    assert len(keys) == 2
    assert {k for k in nn_ops._gn_ws_cache if k[2] == tag} == keys      # one entry per stream, nothing else
    # every workspace is left zero again by the kernels that used it
    assert all(int(nn_ops._gn_ws_cache.pop(k).count_nonzero()) == 0 for k in keys)

    xg = torch.randn(64, 96, device=DEV).to(torch.bfloat16)     # K % 64 != 0: the entry refuses the shape
    with pytest.raises(RuntimeError, match=r"^gd_nn_gemm_forward failed \(-\d+\): gd_nn_gemm_forward: K % 64"):
        nn_ops.gemm(xg, xg)
    with torch.cuda.stream(s):
        with pytest.raises(RuntimeError, match=r"^gd_nn_groupnorm_silu_forward failed \(-\d+\): need C % 8 == 0"):
            nn_ops._GroupNormSiLU.apply(x, w, b, 5, 1e-5, True)  # 32 channels in 5 groups
    torch.cuda.synchronize()
