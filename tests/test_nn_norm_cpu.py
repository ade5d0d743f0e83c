"""CPU half of the norm / softmax / attention gradient tests: the bound of tests/norm_reference.py is proven before
tests/test_nn_norm_gpu.py uses it.  For every case the GPU file runs (its tables are imported, not copied):

  (1) the float64 reference rounded to the kernel's output type (bf16; fp32 for mean / rstd / m1 / m2 / LSE) lies inside the
      bound at every element;
  (2) every wrong formula of ``MUTANTS[op]`` that applies to the case, rounded the same way, leaves the bound by a factor of at
      least 8 at its worst element (over the tensors the operation returns);
  (3) the inputs are what they claim: every (image, group) -- or row -- differs from every other by at least 10 % in mean or
      rstd, and the projection terms are at least 10 % of the plain gradient term in the median.

No kernel runs here, so nothing in this file is measured on the code under test."""
import pytest
import torch

from tests import norm_reference as R
from tests import test_nn_norm_gpu as G

FP32_OUTPUTS = {"mean", "rstd", "m1", "m2", "lse"}
REJECT = 8.0


def _rounded(name, t):
    return t.to(torch.float32).to(torch.float64) if name in FP32_OUTPUTS else R.bf16(t)


def _prove(op, case, label):
    ref = R.call(op, case)
    used = {}
    for name, (r, bound) in R.tensors(ref).items():
        assert bool((bound > 0).all()) and bool(torch.isfinite(r).all()), f"{label} {name}"
        used[name] = R.worst_ratio(_rounded(name, r), r, bound)
        assert used[name] <= 1.0, f"{label} {name}: the rounded float64 reference uses {used[name]:.3f} of its own bound"
    applied = 0
    for mutant, make in R.MUTANTS[op]:
        kw = make(case)
        if kw is None:
            continue
        applied += 1
        wrong = R.tensors(R.call(op, case, **kw))
        worst = max(R.worst_ratio(_rounded(name, wrong[name][0]), *ref[name]) for name in wrong)
        assert worst >= REJECT, f"{label}: '{mutant}' exceeds the bound by only {worst:.2f}x at its worst element"
    assert applied >= 1
    return ref


@pytest.mark.parametrize("case", G.GN_FWD_CASES, ids=G.gn_id)
def test_groupnorm_forward_bound_holds_the_reference_and_rejects_the_mutants(case):
    inp = G.gn_case(*case)
    ref = _prove("gn_forward", inp, f"gn_forward {G.gn_id(case)}")
    assert R.groups_differ(ref["mean"][0], ref["rstd"][0])
    kappa = _kappa(inp)
    assert float(kappa.min()) < 1.5 and float(kappa.max()) > (40.0 if kappa.numel() >= 64 else 20.0) and float(kappa.max()) < 70.0


def _kappa(inp):
    xg = inp["x"].reshape(inp["x"].shape[0], inp["G"], -1)
    return (xg * xg).mean(-1) / xg.var(-1, unbiased=False)


@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("case", G.GN_BWD_CASES, ids=G.gn_id)
def test_groupnorm_backward_bound_holds_the_reference_and_rejects_the_mutants(case, with_add):
    inp = G.gn_case(*case, with_add=with_add)
    ref = _prove("gn_backward", inp, f"gn_backward {G.gn_id(case)} add={with_add}")
    fwd = R.call("gn_forward", inp)
    assert R.groups_differ(fwd["mean"][0], fwd["rstd"][0])
    assert ref["_props"]["m1_share"] >= 0.1 and ref["_props"]["m2_share"] >= 0.1, ref["_props"]


@pytest.mark.parametrize("case", G.LN_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[2]}")
def test_add_layernorm_bounds_hold_the_reference_and_reject_the_mutants(case):
    inp = G.ln_case(*case)
    label = f"add_layernorm {case}"
    fwd = _prove("ln_forward", inp, label + " forward")
    bwd = _prove("ln_backward", inp, label + " backward")
    s = fwd["s"][0]
    assert R.groups_differ(s.mean(-1), (s.var(-1, unbiased=False) + inp["eps"]).rsqrt())
    assert bwd["_props"]["m1_share"] >= 0.1 and bwd["_props"]["m2_share"] >= 0.1, bwd["_props"]


@pytest.mark.parametrize("case", G.SOFTMAX_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_row_softmax_bounds_hold_the_reference_and_reject_the_mutants(case):
    inp = G.softmax_case(*case)
    fwd = _prove("softmax_forward", inp, f"softmax {case} forward")
    p = R.bf16(fwd["p"][0])                      # the backward kernel's input is the forward kernel's bf16 output
    bwd = _prove("softmax_backward", dict(p=p, dp=inp["dp"]), f"softmax {case} backward")
    assert bwd["_props"]["dot_share"] >= 0.1, bwd["_props"]
    assert bool((inp["x"][0] == 3.0).all())                              # the row of equal values
    if case[1] > 8:
        assert bool((fwd["p"][0][1, 1:] == 0).all()) and float(fwd["p"][0][1, 0]) == 1.0      # the row with one finite entry


@pytest.mark.parametrize("case", G.ATTN_CASES, ids=lambda c: f"B{c[0]}H{c[1]}S{c[2]}K{c[3]}" + ("-q0" if c[4] else ""))
def test_attention_bounds_hold_the_reference_and_reject_the_mutants(case):
    B, H, S, Skv, zero_q = case
    inp = G.attention_case(*case)
    label = f"attention {case}"
    fwd = bwd = _prove("attention", inp, label)
    logits = torch.einsum("bshd,bthd->bhst", inp["q"], inp["k"]) / 8.0
    assert float(logits.abs().max()) < 6.0                               # the range the iid tests reach; wide logits are other work
    if zero_q:
        P = torch.exp(logits - fwd["lse"][0][..., None])
        assert float((P - 1.0 / Skv).abs().max()) < 1e-15                # every valid key weighs exactly 1 / Skv
    elif Skv > 1:
        assert bwd["_props"]["D_share"] >= 0.1, bwd["_props"]


def test_one_bf16_step_and_the_caps_on_c():
    assert R.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, -3.0, 0.0], dtype=torch.float64)).tolist() == \
        [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -126]
    x = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 37
    assert bool(((R.bf16(x) - x).abs() <= 0.5 * R.ulp_bf16(x)).all())
    assert max(R.C_GN, R.C_LN, R.C_SOFTMAX) <= 2.0 ** -10 and max(R.C_ATTN, R.C_ATTN_FP32) <= 2.0 ** -7
