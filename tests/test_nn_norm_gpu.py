"""The kernels whose backward pass subtracts a projection -- GroupNorm(+SiLU) in its two-pass and one-launch forms, add +
LayerNorm, row softmax, attention with head dim 64 -- against the float64 statements of tests/norm_reference.py, ELEMENT BY
ELEMENT at the derived bound ``ulp_bf16(ref) + c kappa T`` (never a maximum over the tensor, never a cosine), on inputs where
every (image, group) has its own mean and scale and the upstream gradient is correlated with the normalised input, so that
the projection terms are as large as the gradient itself.  tests/test_nn_norm_cpu.py proves, for exactly these cases (it
imports the tables below), that the bf16-rounded float64 result lies inside the bound and that every wrong formula of
``norm_reference.MUTANTS`` leaves it by a factor of eight or more.

The worst err / bound of every (case, tensor) goes to the parity report.  Nothing here touches the GPU at import."""
import pytest
import torch

from tests import norm_reference as R
from tests.parity_report import record

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G32 = 32

# ---- case tables (shared with the CPU file) -------------------------------------------------------------------------
# C / G = 4, 10, 20, 30, 40, 60, 80 (groups straddle the 8-channel vectors where C / G is no multiple of 8); C / G = 3, which
# the one-launch form refuses; ragged pixel chunks and several statistics chunks per image on the two-pass path
GN_SHAPES = [(2, 128, 2, 2), (3, 320, 3, 5), (2, 640, 4, 4), (1, 960, 8, 8), (2, 1280, 8, 8), (1, 1920, 5, 7), (1, 2560, 8, 8),
             (3, 96, 5, 7), (2, 128, 37, 53)]
GN_FWD_CASES = [(N, C, H, W, silu) for (N, C, H, W) in GN_SHAPES for silu in (True, False)]
# + H W (C // 64) > 16384: the one-launch backward refuses it, the two-pass pair runs on the statistics the one-launch forward kept
GN_BWD_CASES = GN_FWD_CASES + [(1, 640, 48, 48, True)]
LN_CASES = [(rows, C, mode) for (rows, C) in [(5, 320), (77, 640), (130, 1280), (9, 1024)] for mode in ("res+ds", "res", "plain")]
SOFTMAX_CASES = [(9, 8), (5, 264), (3, 1024), (2, 4096)]
# (B, H, S, Skv, q = 0)
ATTN_CASES = [(1, 2, 64, 64, False), (2, 3, 128, 77, False), (1, 2, 192, 65, False), (1, 3, 300, 64, False), (1, 2, 320, 1, False),
              (1, 2, 256, 256, False), (2, 3, 128, 77, True), (1, 2, 192, 65, True)]


def gn_case(N, C, H, W, silu, with_add=False):
    return R.gn_inputs(N, C, H, W, G32, silu, seed=1000 * C + 10 * H + N + int(silu), with_add=with_add)


def ln_case(rows, C, mode):
    case = R.ln_inputs(rows, C, mode != "plain", seed=rows + C)
    if mode != "res+ds":
        case["ds"] = None      # only the LayerNorm's own gradient reaches the node
    return case


def softmax_case(rows, L):
    return R.softmax_inputs(rows, L, seed=rows + L)


def attention_case(B, H, S, Skv, zero_q):
    return R.attention_inputs(B, H, S, Skv, seed=S + Skv + H, zero_q=zero_q)


def gn_id(c):
    return "x".join(str(v) for v in c[:4]) + ("-silu" if c[4] else "-plain")


# ---- comparison ------------------------------------------------------------------------------------------------------
class _Checks:
    """Collects the worst err / bound of every tensor of a case, records it, and fails at the end with all of them."""

    def __init__(self, case):
        self.case, self.rows = case, []

    def add(self, name, got, ref_bound):
        ref, bound = ref_bound
        got = got.detach().to("cpu", torch.float64).reshape(ref.shape)
        ratio = R.worst_ratio(got, ref, bound)
        record(self.case, name, max_err_over_bound=ratio)
        print(f"{self.case} {name}: worst err/bound {ratio:.3f}")
        self.rows.append((name, ratio))

    def finish(self):
        bad = [(n, r) for n, r in self.rows if not r <= 1.0]
        assert not bad, f"{self.case}: outside the bound (worst err / bound): {bad}"


def _nhwc(t, dtype=torch.bfloat16):
    return t.to(DEV, dtype).contiguous(memory_format=torch.channels_last)


def _mr(grad_fn, N):
    mr = grad_fn.saved_tensors[3].detach().to("cpu", torch.float64).view(N, G32, 2)
    return mr[..., 0], mr[..., 1]


def _fused_rules(N, C, H, W):
    """The documented limits of the one-launch kernels (include/gd_nn.h, nn_groupnorm.hip)."""
    cg, total = C // G32, H * W * (C // G32 // 2)
    fwd = cg % 2 == 0 and 4 <= cg <= 128 and total <= 32768 and not (total > 16384 and cg < 16)
    return fwd, fwd and total <= 16384


@pytest.mark.parametrize("case", GN_FWD_CASES, ids=gn_id)
def test_groupnorm_forward_and_kept_statistics_within_the_derived_bound(case):
    """y and the kept mean / rstd of every forward route: no grad (one launch where it fits), with grad (the same launch with
    the statistics kept, or the two-pass pair), and the two-pass pair called directly.  rstd is held to kappa delta / 2, not to
    the rtol of the epilogue-statistics test, which was set for kappa ~ 1."""
    from garmentdreamer_amd import nn_ops
    N, C, H, W, silu = case
    inp = gn_case(*case)
    ref = R.call("gn_forward", inp)
    x, w, b = _nhwc(inp["x"]), inp["gamma"].to(DEV, torch.bfloat16), inp["beta"].to(DEV, torch.bfloat16)
    fwd_ok, _ = _fused_rules(N, C, H, W)
    assert nn_ops.lib().gd_nn_groupnorm_silu_fused_supported(N, H * W, C, G32) == int(fwd_ok)
    chk = _Checks(f"gn_forward {gn_id(case)}")
    with torch.no_grad():
        y0 = nn_ops.group_norm_silu(x, w, b, G32, 1e-5, silu)
    chk.add("y no-grad", y0, ref["y"])
    xg = x.clone().requires_grad_(True)
    y1 = nn_ops.group_norm_silu(xg, w, b, G32, 1e-5, silu)
    assert ("GroupNormSiLUSmall" in type(y1.grad_fn).__name__) == fwd_ok
    chk.add("y grad", y1, ref["y"])
    m, r = _mr(y1.grad_fn, N)
    chk.add("mean grad", m, ref["mean"])
    chk.add("rstd grad", r, ref["rstd"])
    if fwd_ok:
        assert torch.equal(y0, y1.detach())                    # one kernel, statistics kept or not
    y2 = nn_ops._GroupNormSiLU.apply(x.clone().requires_grad_(True), w, b, G32, 1e-5, silu)
    assert "GroupNormSiLUSmall" not in type(y2.grad_fn).__name__
    chk.add("y two-pass", y2, ref["y"])
    m, r = _mr(y2.grad_fn, N)
    chk.add("mean two-pass", m, ref["mean"])
    chk.add("rstd two-pass", r, ref["rstd"])
    chk.finish()


def _gn_two_pass_backward(nn_ops, x, dy, w, b, mr, silu, add):
    N, C, H, W = x.shape
    dx = torch.empty_like(x, memory_format=torch.channels_last)
    ws = nn_ops._gn_workspace(x, N, G32)
    sums = torch.empty(N * G32 * 2, dtype=torch.float32, device=x.device)
    nn_ops._check(nn_ops.lib().gd_nn_groupnorm_silu_backward(
        torch.cuda.current_stream().cuda_stream, x.data_ptr(), dy.data_ptr(), w.data_ptr(), b.data_ptr(), mr.data_ptr(),
        dx.data_ptr(), N, H * W, C, G32, int(silu), ws.data_ptr(), sums.data_ptr(), None if add is None else add.data_ptr()),
        "gd_nn_groupnorm_silu_backward")
    return dx, sums.view(N, G32, 2)


@pytest.mark.parametrize("case", GN_BWD_CASES, ids=gn_id)
def test_groupnorm_backward_routes_within_the_derived_bound(case):
    """dx of the one-launch backward (gn_group_fused_bwd_kernel), of the two-pass pair on kept statistics (gn_bwd_stats_kernel
    + gn_bwd_apply_kernel), and of the two-pass pair with a nonzero ``add`` (the ResnetBlock node's skip gradient), plus the
    group sums m1 / m2 themselves.  Which route ran is asserted; a second call gives the same bits."""
    from garmentdreamer_amd import nn_ops
    N, C, H, W, silu = case
    inp = gn_case(*case, with_add=True)
    add = inp.pop("add")
    ref = R.call("gn_backward", inp)
    ref_add = R.call("gn_backward", inp, add=add)
    x, dy, ad = _nhwc(inp["x"]), _nhwc(inp["dy"]), _nhwc(add)
    w, b = inp["gamma"].to(DEV, torch.bfloat16), inp["beta"].to(DEV, torch.bfloat16)
    fwd_ok, bwd_ok = _fused_rules(N, C, H, W)
    L = nn_ops.lib()
    assert L.gd_nn_groupnorm_silu_fused_supported(N, H * W, C, G32) == int(fwd_ok)
    assert L.gd_nn_groupnorm_silu_fused_backward_supported(N, H * W, C, G32) == int(bwd_ok)
    if (N, C, H, W) == (1, 640, 48, 48):
        assert fwd_ok and not bwd_ok
    if C == 96:
        assert not fwd_ok
    chk = _Checks(f"gn_backward {gn_id(case)}")
    outs = []
    for fn in (lambda t: nn_ops.group_norm_silu(t, w, b, G32, 1e-5, silu), lambda t: nn_ops.group_norm_silu(t, w, b, G32, 1e-5, silu),
               lambda t: nn_ops._GroupNormSiLU.apply(t, w, b, G32, 1e-5, silu)):
        xi = x.clone().requires_grad_(True)
        y = fn(xi)
        mr = y.grad_fn.saved_tensors[3]
        y.backward(dy)
        outs.append((xi.grad, type(y.grad_fn).__name__, mr))
    (dx, name, _), (dx_again, _, _), (dx2, name2, mr2) = outs
    assert ("GroupNormSiLUSmall" in name) == fwd_ok and "GroupNormSiLUSmall" not in name2
    assert torch.equal(dx, dx_again)
    route = "one-launch" if bwd_ok else ("two-pass on one-launch statistics" if fwd_ok else "two-pass")
    chk.add(f"dx dispatch ({route})", dx, ref["dx"])
    chk.add("dx two-pass", dx2, ref["dx"])
    dx3, sums = _gn_two_pass_backward(nn_ops, x, dy, w, b, mr2, silu, ad)
    dx3_again, sums_again = _gn_two_pass_backward(nn_ops, x, dy, w, b, mr2, silu, ad)
    # fp64 atomics of a few fp32 partial sums: exact, so the order of arrival does not show
    assert torch.equal(dx3, dx3_again) and torch.equal(sums, sums_again)
    chk.add("dx two-pass + add", dx3, ref_add["dx"])
    chk.add("m1", sums[..., 0], ref["m1"])
    chk.add("m2", sums[..., 1], ref["m2"])
    chk.add("m1 second call", sums_again[..., 0], ref["m1"])
    chk.add("m2 second call", sums_again[..., 1], ref["m2"])
    chk.finish()


@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_add_layernorm_forward_and_backward_within_the_derived_bound(case):
    """nn_ops.add_layer_norm with a gradient on the activations: s and y of the forward kernel, and d s of
    gd_nn_layernorm_backward -- with a residual and the second gradient arriving on s (the training node), with a residual
    alone, and without a residual."""
    from garmentdreamer_amd import nn_ops
    rows, C, mode = case
    inp = ln_case(*case)
    fwd, bwd = R.call("ln_forward", inp), R.call("ln_backward", inp)
    norm = torch.nn.LayerNorm(C, eps=inp["eps"], device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        norm.weight.copy_(inp["w"].to(DEV, torch.bfloat16))
        norm.bias.copy_(inp["b"].to(DEV, torch.bfloat16))
    norm.requires_grad_(False)
    bf = lambda t: None if t is None else t.to(DEV, torch.bfloat16)     # noqa: E731
    chk = _Checks(f"add_layernorm {rows}x{C}-{mode}")
    grads = []
    for _ in range(2):
        a = bf(inp["x"]).requires_grad_(True)
        r = bf(inp["r"]).requires_grad_(True) if inp["r"] is not None else None
        s_, y_ = nn_ops.add_layer_norm(a, r, norm)
        assert "AddLayerNormTrain" in type(y_.grad_fn).__name__
        if inp["ds"] is not None:
            torch.autograd.backward([y_, s_], [bf(inp["dy"]), bf(inp["ds"])])
        else:
            y_.backward(bf(inp["dy"]))
        grads.append(a.grad)
        if r is not None:
            assert torch.equal(a.grad, r.grad)
    assert torch.equal(grads[0], grads[1])
    with torch.no_grad():
        s0, y0 = nn_ops.add_layer_norm(bf(inp["x"]), bf(inp["r"]), norm)
    assert torch.equal(y0, y_.detach()) and torch.equal(s0, s_.detach())        # the inference call is the same kernel
    chk.add("s", s_, fwd["s"])
    chk.add("y", y_, fwd["y"])
    chk.add("dx", grads[0], bwd["dx"])
    chk.finish()


@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_row_softmax_forward_and_backward_within_the_derived_bound(case):
    """gd_nn_softmax_rows_forward / _backward in place; the backward statement is taken on the kernel's own bf16 p, its input.

    Measured worst err / bound: ds 0.49, p 0.50 on normal numbers; 0.54 (5x264) and 0.66 (3x1024) on p are probabilities of the
    hottest rows that lie below the smallest normal number (1.2e-38): v_exp_f32 returns 0 for them, and the bound at such an
    element is exactly that one flush (norm_reference.ulp_bf16)."""
    from garmentdreamer_amd import nn_ops
    inp = softmax_case(*case)
    chk = _Checks(f"softmax {case[0]}x{case[1]}")
    p = nn_ops.softmax_rows_(inp["x"].to(DEV, torch.bfloat16))
    chk.add("p", p, R.call("softmax_forward", inp)["p"])
    assert torch.isfinite(p.float()).all()
    dp = inp["dp"].to(DEV, torch.bfloat16)
    got = nn_ops.softmax_rows_backward_(p, dp.clone())
    chk.add("ds", got, R.softmax_backward(p.to("cpu", torch.float64), inp["dp"])["ds"])
    assert torch.equal(got, nn_ops.softmax_rows_backward_(p, dp.clone()))
    chk.finish()


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: f"B{c[0]}H{c[1]}S{c[2]}K{c[3]}" + ("-q0" if c[4] else ""))
def test_attention_training_node_within_the_derived_bound(case):
    """nn_ops.attention_d64_train on strided [B, S, H, 64] views of wider projections: o, the LSE, and dq / dk / dv with the
    own backward kernels (_ATTN_BWD = True) and with the library's flash backward on the own LSE (False).  The backward
    statement forms D = rowsum(dO o O) from the bf16 output the node saved (checked against float64 on its own), as both
    backward paths do.  S = 300 is no multiple of 64: the node sends it to the library backward under either setting, which is
    asserted.  With q = 0 every valid key weighs exactly 1 / Skv.  Skv = 1: dq and dk are zero in exact arithmetic, dP - D is then
    the difference of two fp32 sums of the same 64 products in different order (the T2 term of the bound).

    Measured worst err / bound, the same for the own and the library backward: lse 0.06, dv 0.49, o 0.61, dk 0.67, dq 0.81 (all
    at Skv = 77).  Above one half because c is not slack here: P (for o, dv) and dS (for dq, dk) really are rounded to bf16
    before the matrix core, relative 2^-9 each, and where one key carries a row (the hottest head) a single rounding is the
    whole 2^-9 T of the element, with the output's own half step on top; nothing averages out."""
    from garmentdreamer_amd import nn_ops
    B, H, S, Skv, zero_q = case
    inp = attention_case(*case)
    C = H * 64
    wq = torch.randn(B, S, C + 64, device=DEV).to(torch.bfloat16)
    wkv = torch.randn(B, Skv, 2 * C, device=DEV).to(torch.bfloat16)
    wq[..., :C] = inp["q"].reshape(B, S, C).to(DEV, torch.bfloat16)
    wkv[..., :C] = inp["k"].reshape(B, Skv, C).to(DEV, torch.bfloat16)
    wkv[..., C:] = inp["v"].reshape(B, Skv, C).to(DEV, torch.bfloat16)
    q = wq[..., :C].view(B, S, H, 64).detach().requires_grad_(True)
    k = wkv[..., :C].view(B, Skv, H, 64).detach().requires_grad_(True)
    v = wkv[..., C:].view(B, Skv, H, 64).detach().requires_grad_(True)
    assert not q.is_contiguous() and nn_ops.attention_d64_train_supported(q, k, v)
    do = inp["do"].reshape(B, S, C).to(DEV, torch.bfloat16)
    o = nn_ops.attention_d64_train(q, k, v)
    lse = o.grad_fn.saved_tensors[4].clone()
    fwd = R.call("attention_forward", inp)
    name = f"attention B{B}H{H}S{S}K{Skv}" + ("-q0" if zero_q else "")
    chk = _Checks(name)
    chk.add("o", o.view(B, S, H, 64), fwd["o"])
    chk.add("lse", lse, fwd["lse"])
    bwd = R.call("attention_backward", inp, o_saved=o.detach().to("cpu", torch.float64).view(B, S, H, 64))
    L = nn_ops.lib()
    own_kernel, calls, grads = L.gd_nn_attention_d64_backward, [], {}

    def counted(*args):
        calls.append(nn_ops._ATTN_BWD)
        return own_kernel(*args)
    try:
        L.gd_nn_attention_d64_backward = counted
        for own in (True, False):
            nn_ops._ATTN_BWD = own
            grads[own] = torch.autograd.grad(o, (q, k, v), do, retain_graph=True)
    finally:
        nn_ops._ATTN_BWD = True
        L.gd_nn_attention_d64_backward = own_kernel
    assert calls == ([True] if S % 64 == 0 else [])       # which backward ran
    for own in (True, False):
        for key, g in zip(("dq", "dk", "dv"), grads[own]):
            chk.add(f"{key} {'own' if own else 'library'}", g, bwd[key])
    chk.finish()
