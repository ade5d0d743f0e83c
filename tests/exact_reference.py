"""Exact-integer operands, float64 references and the bit comparator of the matrix-core kernel tests.

The NN kernels are linear with fp32 accumulation.  With small-integer operands every product is exact, every partial sum
is exact in any order while its magnitude stays below 2^24, and the final value is exactly representable in bf16 when its
magnitude is at most 256 (128 for half-integers).  The correct output of a kernel is then ONE bit pattern, whatever its
tile shape, split count, summation order or rounding point: the comparison is ``torch.equal`` and a mismatch names the
element.  Plain numpy / torch on the CPU; nothing here touches a GPU.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

SUM_VARIANCE = 1300.0      # bound on the variance of a reduction: standard deviation <= 36.06, see int_operands
F64 = torch.float64


def density(K, var=1.0):
    """Nonzero probability of BOTH multiplied operands of a reduction of length K whose nonzero product terms have mean
    square ``var``: p = min(2/3, sqrt(1300 / (K var))), so that the sum's variance K p^2 var is at most 1300."""
    return min(2.0 / 3.0, math.sqrt(SUM_VARIANCE / (K * var)))


def int_operands(shape, K, rng, lo=-1, hi=1, var=1.0, p=None):
    """Integer-valued float64 tensor of ``shape``.

    K is the full reduction length the tensor takes part in (taps * Cin for a convolution): every element is nonzero
    with probability ``density(K, var)`` and a nonzero element is uniform over the nonzero integers of [lo, hi] (the
    default, lo = -1 and hi = 1: +-1).  K = None draws dense uniform integers of [lo, hi], zero included (bias and
    residual: [-4, 4]).  ``p`` overrides the density where only ONE operand of the product can be thinned (the weights
    behind a GroupNorm loader, whose transformed input is dense); the caller then states its own bound.

    With +-1 operands at density p the sum of K products has variance K p^2 <= 1300: a standard deviation of at most
    36.06.  Over 2^20 outputs the largest |sum| measured on the CPU was 78, 183, 181, 179 and 178 for K = 576, 2880,
    5120, 11520 and 23040 (5.1 standard deviations), so with bias plus residual (at most 8) a reference stays inside
    the 256 that bf16 holds exactly; `assert_exact` checks that for every reference it is given, and
    tests/test_nn_exact_cpu.py for every case of the GPU file.  For +-1 operands the density stays at or above 1/3 up to
    K = 11520, the longest reduction used, so a dropped or misplaced operand element changes tens of outputs; ``var``
    > 1 (operands of a wider range, or a sum that a later stage multiplies again) thins them further."""
    if K is None:
        v = rng.integers(lo, hi + 1, size=shape)
    else:
        values = np.array([i for i in range(lo, hi + 1) if i != 0])
        v = values[rng.integers(0, len(values), size=shape)] * (rng.random(size=shape) < (density(K, var) if p is None else p))
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))


# ---- float64 references ---------------------------------------------------------------------------------------------

def _bias4(b):
    return b[:, :, None, None] if b.dim() == 2 else b[None, :, None, None]


def linear_ref(x, w, bias=None, residual=None, scale=1.0):
    """scale * x w^T + bias + residual."""
    y = (x.to(F64) @ w.to(F64).t()) * scale
    if bias is not None:
        y = y + bias.to(F64)
    if residual is not None:
        y = y + residual.to(F64)
    return y


def conv3x3_ref(x, w, bias=None, residual=None, stride=1, pad_lo=1, scale=1.0):
    """3x3 convolution, zero padding (pad_lo, 1) per axis: stride 1 with pad_lo = 1 is the pad-1 convolution, stride 2
    with pad_lo 0 / 1 the two Downsample2D forms.  bias [Cout] or per image [N, Cout]."""
    xp = F.pad(x.to(F64), (pad_lo, 1, pad_lo, 1))
    y = F.conv2d(xp, w.to(F64), None, stride=stride) * scale
    if bias is not None:
        y = y + _bias4(bias.to(F64))
    if residual is not None:
        y = y + residual.to(F64)
    return y


def conv3x3_dgrad_ref(dy, w, in_hw, stride=1, pad_lo=1):
    """Input gradient of conv3x3_ref: the transposed convolution, cropped to the unpadded input."""
    H, W = in_hw
    Hp, Wp = H + pad_lo + 1, W + pad_lo + 1
    oh, ow = (Hp - 3) // stride + 1, (Wp - 3) // stride + 1
    assert tuple(dy.shape[2:]) == (oh, ow)
    full = F.conv_transpose2d(dy.to(F64), w.to(F64), stride=stride,
                              output_padding=(Hp - ((oh - 1) * stride + 3), Wp - ((ow - 1) * stride + 3)))
    return full[:, :, pad_lo:pad_lo + H, pad_lo:pad_lo + W].contiguous()


def upsample2x_conv3x3_ref(x, w, bias=None):
    """Nearest 2x upsample, then the pad-1 convolution."""
    up = x.to(F64).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    return conv3x3_ref(up, w, bias)


def conv1x1_ref(x, w, bias=None):
    y = F.conv2d(x.to(F64), w.to(F64).reshape(w.shape[0], w.shape[1], 1, 1))
    return y if bias is None else y + _bias4(bias.to(F64))


def conv1x1_dgrad_ref(dy, w):
    return F.conv2d(dy.to(F64), w.to(F64).reshape(w.shape[0], w.shape[1]).t().reshape(w.shape[1], w.shape[0], 1, 1))


def gn_affine_ref(x, mean, rstd, gamma, beta):
    """GroupNorm with supplied statistics and no activation, as the affine map the conv loaders apply:
    x * a + b with a = gamma * rstd and b = beta - mean * a; mean / rstd are [N, groups].  (The convolution reference
    zero-pads AFTER this map: the halo of the transformed tensor is 0, not b.)"""
    N, C = x.shape[:2]
    cg = C // mean.shape[1]
    a = gamma.to(F64)[None, :] * rstd.to(F64).repeat_interleave(cg, dim=1)
    b = beta.to(F64)[None, :] - mean.to(F64).repeat_interleave(cg, dim=1) * a
    return x.to(F64) * a[:, :, None, None] + b[:, :, None, None], a, b


def lora_ref(x, base, down, up, scale, dy=None):
    """y = base + scale * (x down^T) up^T and, with dy, its gradients (dx, d_down, d_up); h = scale * x down^T."""
    x, base, down, up = x.to(F64), base.to(F64), down.to(F64), up.to(F64)
    hs = scale * (x @ down.t())
    out = {"hs": hs, "y": base + hs @ up.t()}
    if dy is not None:
        dy = dy.to(F64)
        dh = scale * (dy @ up)
        out.update(dh=dh, dx=dh @ down, d_down=dh.t() @ x, d_up=dy.t() @ hs)
    return out


# ---- the comparator -------------------------------------------------------------------------------------------------

def check_reference(ref, what, bf16=True):
    """The condition on the reference alone: |ref| < 2^24 (fp32 sums exact) and, for a bf16 output, every value exactly
    representable in bf16.  A failure here is a defect of the test's inputs, not of the kernel."""
    ref = ref.detach().to(F64)
    big = float(ref.abs().max()) if ref.numel() else 0.0
    assert big < 2.0 ** 24, f"{what}: TEST INPUT DEFECT: max |reference| = {big} is not below 2^24"
    if bf16:
        bad = ref != ref.to(torch.bfloat16).to(F64)
        assert not bool(bad.any()), (f"{what}: TEST INPUT DEFECT: {int(bad.sum())} reference values are not representable "
                                     f"in bf16 (max |reference| = {big}); the operands are too dense or too large")
    return ref


def mismatch_report(got, want, what, limit=8):
    """Count, first few indices with got / want, and the per-dimension bounding box of the mismatching indices (the box
    is what tells a tile edge from a halo from a K chunk)."""
    bad = got != want
    idx = bad.nonzero()
    lines = [f"{what}: {idx.shape[0]} of {bad.numel()} elements differ (shape {tuple(got.shape)})"]
    if idx.shape[0]:
        box = ", ".join(f"dim{d}: {int(idx[:, d].min())}..{int(idx[:, d].max())}" for d in range(idx.shape[1]))
        lines.append(f"  bounding box  {box}")
        for i in idx[:limit].tolist():
            lines.append(f"  {tuple(i)}: got {float(got[tuple(i)])}  want {float(want[tuple(i)])}")
    return "\n".join(lines)


def assert_exact(got, ref_f64, what):
    """``got`` (bf16, or fp32 for the LoRA weight gradients and the GroupNorm partial sums; any device, logical NCHW
    indexing) equals the float64 reference bit for bit once the reference is cast to got's type."""
    assert got.dtype in (torch.bfloat16, torch.float32), got.dtype
    ref = check_reference(ref_f64, what, bf16=got.dtype == torch.bfloat16)
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} != reference {tuple(ref.shape)}"
    g = got.detach().cpu()
    want = ref.to(got.dtype)
    assert bool((want.to(F64) == ref).all()), f"{what}: TEST INPUT DEFECT: reference not representable in {got.dtype}"
    # torch.equal: +0 and -0 are the same value; NaN (an element the kernel never wrote) differs from everything
    if not torch.equal(g, want):
        raise AssertionError(mismatch_report(g.to(F64), want.to(F64), what))
