"""Bit-exact tests of the linear matrix-core kernels on small-integer operands (tests/exact_reference.py).

Every kernel here is linear with fp32 accumulation, so on integer operands its correct output is one definite bit pattern:
each comparison is ``assert_exact`` (``torch.equal`` against the float64 reference cast to the output type), never a
tolerance.  A mismatch is a wrong result; its report names the elements and their bounding box.

The operands of a case are a pure function of the case (``*_ops`` below, cached: one reference per case, shared by every
variant / split / entry that runs it).  ``REFERENCES`` lists every operand set with the references the tests compare
against; tests/test_nn_exact_cpu.py imports it and proves on the CPU that each is exactly representable.
"""
import contextlib
import functools
import zlib

import numpy as np
import pytest
import torch

from tests import exact_reference as X
from tests.exact_reference import assert_exact, int_operands

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last


def _rng(kind, *case):
    return np.random.default_rng(zlib.crc32(repr((kind,) + case).encode()))


def _dense(rng, shape, lo=-4, hi=4):
    return int_operands(shape, None, rng, lo, hi)


def bf(t, cl=None):
    """float64 CPU tensor of integers -> bf16 on the device (channels_last for 4-D unless told otherwise)."""
    t = t.to(torch.bfloat16).to(DEV)
    if t.dim() == 4 and cl is not False:
        return t.contiguous(memory_format=CL)
    return t.contiguous()


def poison(ref, dtype=torch.bfloat16):
    """The wrappers allocate their outputs with torch.empty, and the caching allocator hands a freed block to the next
    request of its size -- quite possibly the block that holds the previous variant's correct result.  Fill a block of
    the coming output's size with NaN and free it right before the launch, so an element the kernel never writes
    compares unequal instead of inheriting the right answer."""
    torch.full((ref.numel(),), float("nan"), dtype=dtype, device=DEV)


@contextlib.contextmanager
def forced(variant=-1, split=-1):
    """The library's tuning hooks, restored to the heuristic (-1) whatever happens."""
    from garmentdreamer_amd.nn_ops import lib
    lib().gd_nn_conv_force_variant(variant)
    lib().gd_nn_conv_force_split(split)
    try:
        yield
    finally:
        lib().gd_nn_conv_force_variant(-1)
        lib().gd_nn_conv_force_split(-1)


# =====================================================================================================================
# operand sets (CPU, float64, cached)
# =====================================================================================================================

@functools.lru_cache(maxsize=None)
def conv_ops(N, Cin, Cout, H, W, bias_res, stride=1, pad_lo=1, bias_per_image=True):
    """3x3 convolution (stride 1 / pad 1, or stride 2 with pad (pad_lo, 1)) with its input gradient for an integer dy."""
    rng = _rng("conv", N, Cin, Cout, H, W, bias_res, stride, pad_lo, bias_per_image)
    K = 9 * Cin
    o = {"x": int_operands((N, Cin, H, W), K, rng), "w": int_operands((Cout, Cin, 3, 3), K, rng), "b": None, "r": None}
    if bias_res:
        o["b"] = _dense(rng, (N, Cout) if bias_per_image else (Cout,))
    y = X.conv3x3_ref(o["x"], o["w"], o["b"], None, stride, pad_lo)
    if bias_res and stride == 1:
        o["r"] = _dense(rng, tuple(y.shape))
        y = y + o["r"]
    o["y"] = y
    # density of dy from the gradient's own reduction: 9 taps x Cout channels (stride 2: at most 4 taps reach a pixel)
    o["dy"] = int_operands(tuple(y.shape), 9 * Cout, rng)
    o["dx"] = X.conv3x3_dgrad_ref(o["dy"], o["w"], (H, W), stride, pad_lo)
    return o


@functools.lru_cache(maxsize=None)
def up2_ops(N, Cin, Cout, H, W):
    rng = _rng("up2", N, Cin, Cout, H, W)
    K = 9 * Cin
    o = {"x": int_operands((N, Cin, H, W), K, rng), "w": int_operands((Cout, Cin, 3, 3), K, rng), "b": _dense(rng, (Cout,))}
    o["y"] = X.upsample2x_conv3x3_ref(o["x"], o["w"], o["b"])
    return o


@functools.lru_cache(maxsize=None)
def gn_conv_ops(N, Cin, Cout, H, W, groups, bias_res):
    """GroupNorm in the loader as an exact affine map.  mean: integer in [-2, 2] per (image, group) -- even where rstd is
    0.5, so that mean * a stays integral; rstd in {0.5, 1, 2}; gamma in {-2, -1, 1, 2}; beta an even integer in [-4, 4];
    x even integers.  t = x * a + b is then an integer with |t| <= 2 * 4 + 4 + 2 * 4 = 20, exact in bf16.  t is dense
    (a zero of x maps to b), so only the weights can thin the sum: with m2 = mean(t^2) measured on the reference they are
    +-1 at density p = min(2/3, 1300 / (K m2)), which keeps the variance K p m2 of a sum at or below 1300 as in
    exact_reference.int_operands."""
    rng = _rng("gnconv", N, Cin, Cout, H, W, groups, bias_res)
    K = 9 * Cin
    x = 2.0 * int_operands((N, Cin, H, W), 1, rng)
    rstd = np.array([0.5, 1.0, 2.0])[rng.integers(0, 3, size=(N, groups))]
    mean = rng.integers(-2, 3, size=(N, groups)).astype(np.float64)
    mean = np.where(rstd == 0.5, mean - np.mod(mean, 2), mean)
    gamma = np.array([-2.0, -1.0, 1.0, 2.0])[rng.integers(0, 4, size=(Cin,))]
    beta = 2.0 * rng.integers(-2, 3, size=(Cin,))
    o = {"x": x, "mean": torch.from_numpy(mean), "rstd": torch.from_numpy(rstd), "gamma": torch.from_numpy(gamma),
         "beta": torch.from_numpy(beta.astype(np.float64)), "groups": groups, "b": None, "r": None}
    t, a, b = X.gn_affine_ref(x, o["mean"], o["rstd"], o["gamma"], o["beta"])
    o["t"], o["shift"] = t, b
    m2 = float((t * t).mean())
    o["w"] = int_operands((Cout, Cin, 3, 3), K, rng, p=min(2.0 / 3.0, X.SUM_VARIANCE / (K * m2)))
    if bias_res:
        o["b"], o["r"] = _dense(rng, (N, Cout)), _dense(rng, (N, Cout, H, W))
    o["y"] = X.conv3x3_ref(t, o["w"], o["b"], o["r"])       # the map first, THEN the zero padding
    return o


@functools.lru_cache(maxsize=None)
def first_conv_ops(N, Cin, Cout, H, W):
    rng = _rng("first", N, Cin, Cout, H, W)
    K = 9 * Cin
    o = {"x": int_operands((N, Cin, H, W), K, rng), "w": int_operands((Cout, Cin, 3, 3), K, rng), "b": _dense(rng, (Cout,))}
    o["y"] = X.conv3x3_ref(o["x"], o["w"], o["b"])
    o["dy"] = int_operands(tuple(o["y"].shape), 9 * Cout, rng)
    o["dx"] = X.conv3x3_dgrad_ref(o["dy"], o["w"], (H, W))
    return o


@functools.lru_cache(maxsize=None)
def conv1x1_ops(N, Cin, Cout, H, W):
    rng = _rng("conv1x1", N, Cin, Cout, H, W)
    if Cin == 8:       # quant_conv: eight terms per sum, so dense operands of a wider range
        x, w = _dense(rng, (N, Cin, H, W)), _dense(rng, (Cout, Cin, 1, 1), -2, 2)
        dy = _dense(rng, (N, Cout, H, W))
    else:
        x, w = int_operands((N, Cin, H, W), Cin, rng), int_operands((Cout, Cin, 1, 1), Cin, rng)
        dy = int_operands((N, Cout, H, W), Cout, rng)
    o = {"x": x, "w": w, "b": _dense(rng, (Cout,)), "dy": dy}
    o["y"] = X.conv1x1_ref(x, w, o["b"])
    o["dx"] = X.conv1x1_dgrad_ref(dy, w)
    return o


@functools.lru_cache(maxsize=None)
def linear_ops(M, K, N, bias=True, res=True):
    rng = _rng("linear", M, K, N, bias, res)
    o = {"x": int_operands((M, K), K, rng), "w": int_operands((N, K), K, rng),
         "b": _dense(rng, (N,)) if bias else None, "r": _dense(rng, (M, N)) if res else None}
    o["y"] = X.linear_ref(o["x"], o["w"], o["b"], o["r"])
    o["y_no_res"] = X.linear_ref(o["x"], o["w"], o["b"], None)
    return o


_FP8_VAR = 7.5 * 7.5     # mean square of a product of two nonzero integers uniform on [-4, 4] \ {0}: ((1 + 4 + 9 + 16) / 4)^2


@functools.lru_cache(maxsize=None)
def fp8_linear_ops(M, K, N):
    rng = _rng("fp8lin", M, K, N)
    o = {"x": int_operands((M, K), K, rng, -4, 4, _FP8_VAR), "w": int_operands((N, K), K, rng, -4, 4, _FP8_VAR),
         "b": _dense(rng, (N,)), "r": _dense(rng, (M, N))}
    for dq in (1.0, 0.5):
        o["y", dq] = X.linear_ref(o["x"], o["w"], o["b"], o["r"], scale=dq)
    return o


@functools.lru_cache(maxsize=None)
def fp8_conv_ops(N, Cin, Cout, H, W):
    rng = _rng("fp8conv", N, Cin, Cout, H, W)
    K = 9 * Cin
    o = {"x": int_operands((N, Cin, H, W), K, rng, -4, 4, _FP8_VAR), "w": int_operands((Cout, Cin, 3, 3), K, rng, -4, 4, _FP8_VAR),
         "b": _dense(rng, (N, Cout)), "r": _dense(rng, (N, Cout, H, W))}
    for dq in (1.0, 0.5):
        o["y", dq] = X.conv3x3_ref(o["x"], o["w"], o["b"], o["r"], scale=dq)
    return o


_LORA_VAR = X.SUM_VARIANCE / 16.0     # asks int_operands for K p^2 <= 16: |h| stays near 20, see lora_ops


@functools.lru_cache(maxsize=None)
def lora_ops(M, K, N):
    """y = base + 0.5 * (x down^T) up^T.  down and up are EVEN integers (+-2), so 0.5 * x . down and 0.5 * dy . up are
    integers.  The rank-4 update multiplies h by up and sums four terms, so h must stay small for y to fit bf16: the
    densities are chosen for a variance of 16 of h and dh (|h| <= ~20), which bounds |y| and |dx| by 4 + 4 * 2 * 20."""
    rng = _rng("lora", M, K, N)
    o = {"x": int_operands((M, K), K, rng, var=_LORA_VAR), "down": 2.0 * int_operands((4, K), K, rng, var=_LORA_VAR),
         "up": 2.0 * int_operands((N, 4), N, rng, var=_LORA_VAR), "base": _dense(rng, (M, N)),
         "dy": int_operands((M, N), N, rng, var=_LORA_VAR), "w": int_operands((N, K), K, rng, var=_LORA_VAR)}
    o.update(X.lora_ref(o["x"], o["base"], o["down"], o["up"], 0.5, o["dy"]))
    o["y_linear"] = X.linear_ref(o["x"], o["w"]) + o["hs"] @ o["up"].t()       # lora_linear: the frozen projection as base
    o["xw"] = X.linear_ref(o["x"], o["w"])
    return o


# =====================================================================================================================
# case tables
# =====================================================================================================================
VARIANTS = [0, 1, 2, 4, 5, 6, 7]          # launch_conv's tiles: 128x128, 128x256, 256x256, 32x256, 64x128, 64x64, 128x64

# N, Cin, Cout, H, W, bias + residual.  M = 351 is ragged against 64, 128 and 256 and its tiles straddle image boundaries;
# Cout = 72 is ragged against 32 .. 256, 264 is one full 256-channel tile plus 8 channels
IGEMM_CASES = [(3, 128, 72, 9, 13, True), (3, 128, 264, 9, 13, False)]
IGEMM_DEEP = (2, 1280, 72, 8, 8, True)    # K = 11520: 20 K-steps per tap, a split range cuts a tap in the middle
PATCH_CASES = [(2, 128, 72, 17, 23, True, -1), (2, 128, 256, 17, 23, True, -1), (2, 128, 256, 17, 23, True, 0)]
TILED_CASES = [(2, 96, Cout, 17, 33, br) for Cout in (72, 136) for br in (False, True)]
# kind, N, Cin, Cout, H, W, groups, bias + residual
GN_CASES = [(kind, 2, 128, 72, 17, 33 if kind != "patch" else 23, 32, False) for kind in ("wide", "wino", "patch")] + \
           [(kind, 2, 320, 136, 17, 33 if kind != "patch" else 23, 32, True) for kind in ("wide", "wino", "patch")]
S2_CASES = [(2, 128, 192, 9, 13, 0), (2, 128, 192, 9, 13, 1)]
S2_FWD_CASES = [(2, 128, 72, 9, 13, 0), (2, 128, 72, 9, 13, 1)]
UP2_CASE = (2, 64, 72, 5, 7)
FIRST_CASES = [(3, 3, 128, 9, 37), (3, 4, 128, 9, 37), (3, 3, 192, 9, 37)]
C8_CASE = (3, 8, 8, 17, 5)
CONV1X1_CASE = (2, 128, 72, 9, 13)
LINEAR_CASE = (351, 128, 72)
LINEAR_320_CASES = [(4096 + 300, 320), (4096 + 33, 320), (4096 + 33, 640)]
GEMM_CASES = [(513, 64, 264), (300, 320, 8), (77, 1024, 320), (65792, 64, 320)]
FP8_LINEAR_CASE = (351, 320, 72)
FP8_CONV_CASE = (2, 320, 72, 9, 13)
LORA_CASES = [(M, K, N) for M in (154, 1001) for K, N in ((1024, 320), (320, 320))]
LORA_GROUP = [(154, 1024, 320), (1001, 320, 320)]


def _refs(o, bf16=(), fp32=()):
    return [(k, o[k], True) for k in bf16] + [(k, o[k], False) for k in fp32]


def _references():
    """(id, thunk) per operand set; the thunk returns [(name, float64 reference, output is bf16)] -- every reference a GPU
    test below hands to assert_exact."""
    out = []
    for c in IGEMM_CASES + [IGEMM_DEEP]:
        out.append((f"conv-{c}", lambda c=c: _refs(conv_ops(*c), ("y", "dx"))))
    for c in sorted({c[:6] for c in PATCH_CASES}) + TILED_CASES:
        out.append((f"conv-{c}", lambda c=c: _refs(conv_ops(*c), ("y",))))
    for c in sorted({c[1:] for c in GN_CASES}):
        out.append((f"gnconv-{c}", lambda c=c: _refs(gn_conv_ops(*c), ("t", "y"))))
    for c in S2_CASES:
        out.append((f"s2-{c}", lambda c=c: _refs(conv_ops(*c[:5], True, 2, c[5], False), ("y", "dx"))))
    for c in S2_FWD_CASES:
        out.append((f"s2fwd-{c}", lambda c=c: _refs(conv_ops(*c[:5], True, 2, c[5], False), ("y",))))
    out.append((f"up2-{UP2_CASE}", lambda: _refs(up2_ops(*UP2_CASE), ("y",))))
    for c in FIRST_CASES:
        out.append((f"first-{c}", lambda c=c: _refs(first_conv_ops(*c), ("y", "dx"))))
    for c in (C8_CASE, CONV1X1_CASE):
        out.append((f"conv1x1-{c}", lambda c=c: _refs(conv1x1_ops(*c), ("y", "dx"))))
    out.append((f"linear-{LINEAR_CASE}", lambda: _refs(linear_ops(*LINEAR_CASE), ("y", "y_no_res"))))
    for M, N in LINEAR_320_CASES:
        for bias in (True, False):
            out.append((f"linear320-{(M, N, bias)}", lambda M=M, N=N, bias=bias: _refs(linear_ops(M, 320, N, bias, False), ("y",))))
    for c in GEMM_CASES:
        out.append((f"gemm-{c}", lambda c=c: _refs(linear_ops(*c), ("y", "y_no_res"))))
    out.append((f"fp8linear-{FP8_LINEAR_CASE}", lambda: _refs(fp8_linear_ops(*FP8_LINEAR_CASE), (("y", 1.0), ("y", 0.5)))))
    out.append((f"fp8conv-{FP8_CONV_CASE}", lambda: _refs(fp8_conv_ops(*FP8_CONV_CASE), (("y", 1.0), ("y", 0.5)))))
    for c in sorted(set(LORA_CASES + LORA_GROUP)):
        out.append((f"lora-{c}", lambda c=c: _refs(lora_ops(*c), ("y", "dx", "y_linear", "xw"), ("hs", "dh", "d_down", "d_up"))))
    return out


REFERENCES = _references()


# =====================================================================================================================
# implicit-GEMM convolution: every tile variant, forced splits, input gradient
# =====================================================================================================================

def _conv_args(o):
    return bf(o["x"]), bf(o["w"]), None if o["b"] is None else bf(o["b"]), None if o["r"] is None else bf(o["r"])


@pytest.mark.parametrize("case", IGEMM_CASES, ids=str)
@pytest.mark.parametrize("variant", VARIANTS)
def test_implicit_gemm_conv_is_exact_on_every_tile_variant(variant, case):
    """nn_ops._conv_launch with gd_nn_conv_force_variant(v).  The split is forced to 1 together with the variant: left to
    the heuristic, a shape this small runs split-K, and a split launch picks its own tile and ignores the forced one."""
    from garmentdreamer_amd import nn_ops
    o = conv_ops(*case)
    x, w, b, r = _conv_args(o)
    with forced(variant=variant, split=1):
        poison(o["y"])
        y = nn_ops._conv_launch(x, w, b, r, case[2])
    assert_exact(y, o["y"], f"conv3x3 variant {variant} {case}")


@pytest.mark.parametrize("case", IGEMM_CASES + [IGEMM_DEEP], ids=str)
@pytest.mark.parametrize("split", [1, 2, 7])
def test_implicit_gemm_conv_is_exact_under_forced_splits(split, case):
    from garmentdreamer_amd import nn_ops
    o = conv_ops(*case)
    x, w, b, r = _conv_args(o)
    with forced(split=split):
        poison(o["y"])
        y = nn_ops._conv_launch(x, w, b, r, case[2])
    assert_exact(y, o["y"], f"conv3x3 split {split} {case}")


@pytest.mark.parametrize("case", IGEMM_CASES + [IGEMM_DEEP], ids=str)
@pytest.mark.parametrize("split", [-1, 2])
def test_conv3x3_input_gradient_is_exact(split, case):
    """conv3x3(...).backward with an integer dy: the transposed convolution on the flipped weights (Cout = 72 and 264 are no
    multiples of 64, so the gradient's K is zero-padded to the next K-step), default route and forced split 2."""
    from garmentdreamer_amd import nn_ops
    o = conv_ops(*case)
    x, w, b, r = _conv_args(o)
    x.requires_grad_(True)
    with forced(split=split):
        poison(o["y"])
        y = nn_ops.conv3x3(x, w, b, r)
        poison(o["dx"])
        y.backward(bf(o["dy"]))
    assert_exact(y, o["y"], f"conv3x3 forward (split {split}) {case}")
    assert_exact(x.grad, o["dx"], f"conv3x3 input gradient (split {split}) {case}")


# =====================================================================================================================
# patch-staged kernel
# =====================================================================================================================

@pytest.mark.parametrize("case", PATCH_CASES, ids=str)
def test_patch_staged_conv_is_exact(case):
    """One full 16x16 patch plus ragged patches on both edges; a ragged 128-channel slab (Cout = 72), the 256-channel slab,
    and (force-variant 0) the 128-channel slab kernel on a two-slab layer."""
    from garmentdreamer_amd import nn_ops
    o = conv_ops(*case[:6])
    x, w, b, r = _conv_args(o)
    with forced(variant=case[6]):
        poison(o["y"])
        y = nn_ops._patch_launch(x, w, b, r, case[2])
    assert_exact(y, o["y"], f"patch conv {case}")


# =====================================================================================================================
# wide-tile and Winograd kernels
# =====================================================================================================================

@pytest.mark.parametrize("case", TILED_CASES, ids=str)
@pytest.mark.parametrize("kernel", ["wide", "wino"])
def test_wide_and_winograd_convs_and_their_statistics_are_exact(kernel, case):
    """Ragged against the 16x32 pixel tile in both directions, Cin = 96 (three 32-channel chunks), ragged channel tiles.

    Winograd F(2,3) along x is exact here as well: the filter transform is 0.5 * ((g0 + g2) +- g1) (and g0, g2
    themselves); with weights in {-1, 0, 1} that is a half-integer of magnitude at most 1.5, exact in bf16.  The
    transformed inputs are differences of two inputs in {-1, 0, 1}: integers of magnitude at most 2.  Products and fp32
    sums of those are exact, and the output transform adds and subtracts exact values, so the kernel must reproduce the
    direct convolution's bits.

    stat_part: the epilogue's partial sums of y and y^2, summed over the rows in float64, equal the sums over the stored
    output exactly (integers; the test first asserts that the totals, which bound every partial, are below 2^24)."""
    from garmentdreamer_amd import nn_ops
    N, Cin, Cout, H, W, _ = case
    o = conv_ops(*case)
    x, w, b, r = _conv_args(o)
    rows = ((H + 15) // 16) * ((W + 15) // 16) * 8
    part = torch.full((N * (Cout // 4) * rows * 2,), float("nan"), dtype=torch.float32, device=DEV)
    launch = nn_ops._wide_launch if kernel == "wide" else nn_ops._wino_launch
    poison(o["y"])
    y = launch(x, w, b, r, Cout, part)
    assert_exact(y, o["y"], f"{kernel} conv {case}")
    yq = o["y"].view(N, Cout // 4, 4, H * W)
    want = torch.stack([yq.sum((2, 3)), (yq * yq).sum((2, 3))], -1)
    assert float(want.abs().max()) < 2.0 ** 24
    assert bool(torch.isfinite(part).all()), "a statistics row was never written"
    got = part.view(N, Cout // 4, rows, 2).double().sum(2).cpu()
    assert torch.equal(got, want), X.mismatch_report(got, want, f"{kernel} epilogue statistics {case}")


@pytest.mark.parametrize("case", GN_CASES, ids=str)
def test_groupnorm_in_the_conv_loader_is_an_exact_affine_map(case):
    """Wide, Winograd and patch GroupNorm entries with statistics built by the test (gn_conv_ops), silu = 0.  Pins the
    per-(image, group) indexing of the statistics, the per-channel indexing of a / b in every channel chunk (Cin = 320:
    10-channel groups that straddle the 32- and 64-channel chunks), and that the halo is zero AFTER the transform."""
    from garmentdreamer_amd import nn_ops
    kind, N, Cin, Cout, H, W, groups, _ = case
    o = gn_conv_ops(*case[1:])
    x, w, b, r = _conv_args(o)
    mr = torch.stack([o["mean"], o["rstd"]], -1).reshape(-1).float().to(DEV).contiguous()
    gn = (mr, bf(o["gamma"]), bf(o["beta"]), groups, 0)
    poison(o["y"])
    y = nn_ops._tiled_launch(kind, x, w, b, r, Cout, gn=gn)
    assert_exact(y, o["y"], f"{kind} GroupNorm conv {case}")


# =====================================================================================================================
# other convolution forms
# =====================================================================================================================

@pytest.mark.parametrize("case", S2_CASES, ids=str)
def test_stride2_conv_and_its_input_gradient_are_exact(case):
    """conv3x3_s2 with pad_lo 0 and 1.  The wrapper (and the gradient entry) need Cout % 64 == 0 and refuse the 72 output
    channels of the stride-1 cases: 192 is the nearest count that is still ragged against the 128- and 256-channel tiles;
    the forward entry alone takes Cout = 72 (next test)."""
    from garmentdreamer_amd import nn_ops
    N, Cin, Cout, H, W, pad_lo = case
    o = conv_ops(N, Cin, Cout, H, W, True, 2, pad_lo, False)
    x, w, b, _ = _conv_args(o)
    x.requires_grad_(True)
    poison(o["y"])
    y = nn_ops.conv3x3_s2(x, w, b, pad_lo)
    poison(o["dx"])
    y.backward(bf(o["dy"]))
    assert_exact(y, o["y"], f"conv3x3_s2 {case}")
    assert_exact(x.grad, o["dx"], f"conv3x3_s2 input gradient {case}")


@pytest.mark.parametrize("case", S2_FWD_CASES, ids=str)
def test_stride2_conv_forward_is_exact_on_a_ragged_channel_tile(case):
    from garmentdreamer_amd import nn_ops
    N, Cin, Cout, H, W, pad_lo = case
    o = conv_ops(N, Cin, Cout, H, W, True, 2, pad_lo, False)
    x, w, b, _ = _conv_args(o)
    with torch.no_grad():
        poison(o["y"])
        y = nn_ops._Conv3x3S2.apply(x, w, b, pad_lo)
    assert_exact(y, o["y"], f"conv3x3_s2 forward {case}")


def test_upsample_fused_conv_is_exact():
    """The four parity classes use pre-summed weights: sums of up to four values in {-1, 0, 1} are exact in bf16."""
    from garmentdreamer_amd import nn_ops
    o = up2_ops(*UP2_CASE)
    with torch.no_grad():
        y = nn_ops.upsample2x_conv3x3(bf(o["x"]), bf(o["w"]), bf(o["b"]))
    assert_exact(y, o["y"], f"upsample2x_conv3x3 {UP2_CASE}")


@pytest.mark.parametrize("case", FIRST_CASES, ids=str)
def test_first_conv_and_its_input_gradient_are_exact(case):
    """conv3x3_small_cin: the matrix-core first convolution (Cout = 128, Cin 3 and 4) and the generic kernel (Cout = 192);
    input gradient through csrc/nn_conv_first_dgrad.h (Cin = 3, Cout = 128) and the padded implicit-GEMM form otherwise."""
    from garmentdreamer_amd import nn_ops
    o = first_conv_ops(*case)
    x = bf(o["x"]).requires_grad_(True)
    w, b = bf(o["w"]), bf(o["b"])
    poison(o["y"])
    y = nn_ops.conv3x3_small_cin(x, w, b)
    assert not nn_ops.library_fallbacks().get("conv3x3_small_cin")
    y.backward(bf(o["dy"]))
    assert_exact(y, o["y"], f"first conv {case}")
    assert_exact(x.grad, o["dx"], f"first conv input gradient {case}")


def test_conv1x1_forms_are_exact():
    from garmentdreamer_amd import nn_ops
    o = conv1x1_ops(*C8_CASE)
    x, w, b = bf(o["x"]).requires_grad_(True), bf(o["w"], cl=False), bf(o["b"])
    assert nn_ops.conv1x1_c8_supported(x, w, b)
    y = nn_ops.conv1x1_c8(x, w, b)
    y.backward(bf(o["dy"]))
    assert_exact(y, o["y"], f"conv1x1_c8 {C8_CASE}")
    assert_exact(x.grad, o["dx"], f"conv1x1_c8 input gradient {C8_CASE}")
    o = conv1x1_ops(*CONV1X1_CASE)
    y = nn_ops.conv1x1(bf(o["x"]), bf(o["w"], cl=False), bf(o["b"]))
    assert_exact(y, o["y"], f"conv1x1 {CONV1X1_CASE}")


# =====================================================================================================================
# linears
# =====================================================================================================================

@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("variant", [-1] + VARIANTS)
def test_one_tap_linear_is_exact_on_every_tile_variant(variant, res):
    from garmentdreamer_amd import nn_ops
    o = linear_ops(*LINEAR_CASE)
    x, w, b = bf(o["x"]), bf(o["w"]), bf(o["b"])
    assert nn_ops.linear_supported(x, w)
    with forced(variant=variant), torch.no_grad():
        poison(o["y"])
        y = nn_ops.linear(x, w, b, bf(o["r"]) if res else None)
    assert_exact(y, o["y"] if res else o["y_no_res"], f"linear variant {variant} residual {res}")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("M,N", LINEAR_320_CASES)
def test_linear_320_is_exact(M, N, bias):
    """The streaming K = 320 kernel takes 4096 rows or more (gd_nn_linear_320_supported), so the short ragged row count is
    4096 + 300 rather than 300: the same 300-row remainder behind full row tiles."""
    from garmentdreamer_amd import nn_ops
    o = linear_ops(M, 320, N, bias, False)
    x, w, b = bf(o["x"]), bf(o["w"]), bf(o["b"]) if bias else None
    assert nn_ops.linear_320_supported(x, w, b)
    poison(o["y"])
    assert_exact(nn_ops.linear_320(x, w, b), o["y"], f"linear_320 {(M, N, bias)}")


@pytest.mark.parametrize("M,K,N", GEMM_CASES)
def test_own_gemm_is_exact(M, K, N):
    """Ragged rows and channels with one K tile; one narrow channel tile with five K tiles; sixteen K tiles; and 514 tiles,
    more than one pass of the persistent grid.  Bias and residual are the accumulators' starting value."""
    from garmentdreamer_amd import nn_ops
    o = linear_ops(M, K, N)
    x, w, b, r = bf(o["x"]), bf(o["w"]), bf(o["b"]), bf(o["r"])
    assert nn_ops.gemm_supported(x, w, b, r)
    poison(o["y"])
    assert_exact(nn_ops.gemm(x, w, b, r), o["y"], f"gemm + bias + residual {(M, K, N)}")
    poison(o["y"])
    assert_exact(nn_ops.gemm(x, w, b), o["y_no_res"], f"gemm + bias {(M, K, N)}")


def _e4m3_bytes(t):
    return t.float().to(torch.float8_e4m3fn).view(torch.uint8)


@pytest.mark.parametrize("dq", [1.0, 0.5])
def test_fp8_linear_is_exact(dq):
    """Integers in [-4, 4] are exact in e4m3: quantised and packed with scale 1 they come back byte for byte (torch's own
    float8_e4m3fn cast).  K = 320 packs to Kp = 384, so the zero-padded K tail is read."""
    from garmentdreamer_amd import nn_ops
    M, K, N = FP8_LINEAR_CASE
    o = fp8_linear_ops(M, K, N)
    x, w = bf(o["x"]), bf(o["w"])
    x8, w8 = nn_ops.fp8_quantize(x, 1.0), nn_ops.fp8_pack_weights(w, 1.0)
    assert torch.equal(x8, _e4m3_bytes(x))
    assert w8.shape == (N, 384) and torch.equal(w8[:, :K], _e4m3_bytes(w)) and int(w8[:, K:].max()) == 0
    poison(o["y", dq])
    y = nn_ops.fp8_linear(x8, w8, bf(o["b"]), bf(o["r"]), K, dq)
    assert_exact(y, o["y", dq], f"fp8_linear dq {dq}")


@pytest.mark.parametrize("dq", [1.0, 0.5])
def test_fp8_conv3x3_is_exact(dq):
    from garmentdreamer_amd import nn_ops
    N, Cin, Cout, H, W = FP8_CONV_CASE
    o = fp8_conv_ops(*FP8_CONV_CASE)
    x, w = bf(o["x"]), bf(o["w"])
    x8 = nn_ops.fp8_quantize(x.permute(0, 2, 3, 1), 1.0).permute(0, 3, 1, 2)          # NHWC bytes viewed as [N, C, H, W]
    w2d = w.permute(0, 2, 3, 1).reshape(Cout * 9, Cin)                                  # [Cout][3][3][Cin]
    w8 = nn_ops.fp8_pack_weights(w2d, 1.0)
    assert torch.equal(x8, _e4m3_bytes(x)) and torch.equal(w8[:, :Cin], _e4m3_bytes(w2d)) and int(w8[:, Cin:].max()) == 0
    poison(o["y", dq])
    y = nn_ops.fp8_conv3x3(x8, w8, bf(o["b"]), bf(o["r"]), Cin, dq)
    assert_exact(y, o["y", dq], f"fp8_conv3x3 dq {dq}")


# =====================================================================================================================
# LoRA
# =====================================================================================================================

def _lora_args(o):
    return (bf(o["x"]), bf(o["base"]), o["down"].float().to(DEV).contiguous(), o["up"].float().to(DEV).contiguous(),
            bf(o["dy"]))


@pytest.mark.parametrize("M,K,N", LORA_CASES)
def test_lora_forward_kernels_are_exact(M, K, N):
    from garmentdreamer_amd import nn_ops
    o = lora_ops(M, K, N)
    x, base, down, up, dy = _lora_args(o)
    hs = nn_ops._lora_rowdot(x, down, 0.5, 0)
    assert_exact(hs, o["hs"], f"lora rowdot {(M, K, N)}")
    assert_exact(nn_ops._lora_rank4_add(hs, up, base, N, 1), o["y"], f"lora rank4_add {(M, K, N)}")
    y, h = nn_ops._lora_row_fused(x, down, up, base, N, 0.5, 0)
    assert_exact(h, o["hs"], f"lora row_fused h {(M, K, N)}")
    assert_exact(y, o["y"], f"lora row_fused y {(M, K, N)}")
    # the backward form of the same kernels: a = dy, w1 = up [N][4], w2 = down [4][K]
    dh = nn_ops._lora_rowdot(dy, up, 0.5, 1)
    assert_exact(dh, o["dh"], f"lora rowdot (backward form) {(M, K, N)}")
    assert_exact(nn_ops._lora_rank4_add(dh, down, None, K, 0), o["dx"], f"lora rank4_add (backward form) {(M, K, N)}")


@pytest.mark.parametrize("M,K,N", LORA_CASES)
def test_lora_branch_and_its_gradients_are_exact(M, K, N):
    """dx in bf16, d_down and d_up in fp32.  The column reductions over M are integer sums (the references are asserted
    below 2^24), so the chunked order cannot matter."""
    from garmentdreamer_amd import nn_ops
    o = lora_ops(M, K, N)
    x, base, down, up, dy = _lora_args(o)
    for t in (x, base, down, up):
        t.requires_grad_(True)
    assert nn_ops.lora_branch_supported(x, base, down, up)
    poison(o["y"])
    y = nn_ops.lora_branch(x, base, down, up, 0.5)
    poison(o["dx"])
    y.backward(dy)
    assert_exact(y, o["y"], f"lora_branch y {(M, K, N)}")
    assert_exact(x.grad, o["dx"], f"lora_branch dx {(M, K, N)}")
    assert torch.equal(base.grad, dy)
    assert_exact(down.grad, o["d_down"], f"lora_branch d_down {(M, K, N)}")
    assert_exact(up.grad, o["d_up"], f"lora_branch d_up {(M, K, N)}")


def test_grouped_lora_weight_gradients_are_exact():
    """lora_grad_group with two adapters of different shapes: one grouped launch per stage into the optimizer's sinks."""
    from garmentdreamer_amd import nn_ops
    from garmentdreamer_amd.flat_adam import FlatAdam
    import torch.nn.functional as F
    layers = []
    for c in LORA_GROUP:
        o = lora_ops(*c)
        x, _, down, up, dy = _lora_args(o)
        layers.append((o, x.requires_grad_(True), bf(o["w"]), torch.nn.Parameter(down), torch.nn.Parameter(up), dy))
    params = [p for _, _, _, d, u, _ in layers for p in (d, u)]
    opt = FlatAdam(params, lr=1e-3, flat=params)
    opt.zero_grad()
    with nn_ops.lora_grad_group() as grp:
        ys = [nn_ops.lora_linear(x, w, d, u, 0.5, (lambda t, w=w: F.linear(t, w))) for _, x, w, d, u, _ in layers]
    torch.autograd.backward(ys, [dy for *_, dy in layers])
    torch.cuda.synchronize()
    assert grp is not None and grp.expected == 2 and grp.launches == 1 and nn_ops.lora_groups_pending() == 0
    for (o, x, w, d, u, dy), y, c in zip(layers, ys, LORA_GROUP):
        assert_exact(y, o["y_linear"], f"lora_linear y {c}")
        assert_exact(d.grad, o["d_down"], f"grouped d_down {c}")
        assert_exact(u.grad, o["d_up"], f"grouped d_up {c}")
