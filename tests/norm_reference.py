"""Float64 statements of the kernels whose backward pass subtracts a projection (GroupNorm(+SiLU), add + LayerNorm, row
softmax, attention with head dim 64), the structured inputs that make every projection term O(1), a list of named WRONG
formulas on the same inputs (``MUTANTS``), and the per-element error bound the GPU tests assert:

    bound(e) = ulp_bf16(ref(e)) + c * kappa * T(e)

``ulp_bf16`` is one bf16 step at |ref(e)| (the output's own rounding), ``T(e)`` is the sum of the absolute values of the
terms of element e BEFORE they cancel, ``c`` stands for the kernel's internal arithmetic and is derived per kernel below,
``kappa = E[x^2] / var = 1 + mean^2 / var`` of the element's group multiplies c only for GroupNorm, whose statistics come
from a one-pass variance.  Plain float64 torch on the CPU; nothing here imports the package under test.

Every function returns a dict ``{name: (ref, bound)}`` of float64 tensors in the layout the kernel uses.
"""
import math

import torch

F64 = torch.float64

# ---------------------------------------------------------------------------------------------------------------------
# the constants c, with their derivations (u = 2^-24, the fp32 unit roundoff)
# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm statistics: a sum passes through at most n fp32 additions before the fp64 stage.  Two-pass kernels
# (gn_stats_kernel / gn_bwd_stats_kernel -> reduce_to_groups): ceil(ppb_stats / rows) pixels per thread, then `rows` LDS rows,
# then C/G channels -- at most 1 + 1 + 80 = 82 on the shapes of tests/test_nn_norm_gpu.py ((1, 2560, 8, 8)); one-launch kernels:
# R <= 32 registers per accumulator.  n <= 128, each addition errs by at most u of the running sum of magnitudes:
GN_DELTA = 2.0 ** -17           # = 128 u: relative error of a group's fp32 partial sums (of x, x^2, gamma dz, gamma dz xhat)
# var = E[x^2] - mean^2 in fp64 from those sums: d var <= delta E[x^2] = delta kappa var, so d rstd / rstd <= kappa delta / 2;
# rsqrtf, the fp32 cast of var and the + eps add 3 more roundings of ~1 ulp (2^-23 each)
GN_RSTD_EXTRA = 2.0 ** -21
# GroupNorm elementwise chain in fp32: xhat = (x - mean) rstd, z = gamma xhat + beta, sigmoid = rcp(1 + exp2(-z log2 e))
# (v_exp_f32, v_rcp_f32: ~1 ulp = 2^-23 each), silu' = sg (1 + z (1 - sg)), gamma dz - m1 - xhat m2, * rstd: <= 16 roundings
# = 2^-20.  The statistics enter every term: kappa delta / 2 (rstd) + delta (m1, m2) <= 1.5 kappa 2^-17.  Total
# <= kappa (1.5 * 2^-17 + 2^-20) = 0.81 kappa 2^-16; the rest of c = 2^-16 takes the fp32 rounding of mean (2^-24 sqrt(kappa - 1)
# in xhat) and of m1 / m2 (2^-24).  Under the 2^-10 cap for an fp32-internal kernel by a factor 64.
C_GN = 2.0 ** -16
# LayerNorm (one wave per row, two-pass variance in registers: no kappa): per-lane fp32 sums of <= 8 VPL = 32 elements and six
# shuffle levels, so mean / var / m1 / m2 err by <= 38 u of their magnitude sums; mean's error reaches xhat as
# 38 u mean|s| rstd, which T carries through its |mean| term.  The chain (s - mean) rstd w + b / (a - ma - xhat mb) rstd + ds is
# <= 8 roundings.  Total <= (38 * 3 + 8) u < 2^-17; c = 2^-16 leaves a factor 2.
C_LN = 2.0 ** -16
# Row softmax (one wave per row, fp32): exp2(x k - m k): the argument errs by <= 2 u (|x| + |m|) log2 e, i.e. p by
# <= 2 u (|x| + |m|) -- T carries (|x| + |m|) / 64 for it, c / 64 = 2^-20 = 16 u; v_exp_f32 1 ulp; the row sum is <= 64 elements
# per lane + six shuffle levels = 70 u; 1 / sum and the product 2 roundings.  Total <= 80 u < 2^-17.  Backward: the dot product
# sum(p dp) the same 70 u of sum |p dp| (in T), two more roundings.
C_SOFTMAX = 2.0 ** -14
# Attention (head dim 64).  "P and dS are rounded to bf16 where they enter an MFMA" (nn_attention.hip): one bf16 rounding,
# relative 2^-9, of every P (forward P V, backward dV = P^T dO) or dS (dQ = dS K / 8, dK = dS^T Q / 8) term: 2^-9 T.  P itself
# = exp2(s c - L) in fp32: argument error <= u (|s c| + |L|) * 3 < 2^-18 for logits below 16, v_exp_f32 2^-23; the forward
# divides by an fp32 row sum of Skv terms (Skv u).  Everything fp32 together < 2^-12.  c = 2^-9 + 2^-12, under the 2^-7 cap.
C_ATTN = 2.0 ** -9 + 2.0 ** -12
# dP - D cancels BEFORE it is multiplied by P (exactly, when there is one key): both are fp32 sums of 64 products, dP inside the
# matrix core, D in attn_dsum_kernel: 2 * 64 u of sum_d |dO_d| (|v_kd| + |o_d|), which the second magnitude T2 carries.
C_ATTN_FP32 = 2.0 ** -16
# LSE = m c ln 2 + ln l in fp32: scores are fp32 sums of 64 products (64 u = 2^-18 of sum |q k| / 8), l a sum of Skv fp32 terms
# (Skv u, as an absolute error of ln l), __logf ~2^-21 absolute, the products and the final add 4 roundings of |lse| + |m|.
C_LSE_SCORE = 2.0 ** -18


def bf16(t):
    """Round to bf16 (nearest even), back in float64."""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def ulp_bf16(ref):
    """One bf16 step at |ref|: 2^(e - 7) for 2^e <= |ref| < 2^(e + 1).  Never below 2^-126, the smallest normal number: the
    kernels may flush a subnormal result to zero (v_exp_f32 returns no denormals: a probability below 1.2e-38 comes out as 0)."""
    ref = ref.to(F64)
    _, e = torch.frexp(ref.abs())
    e = torch.where(ref == 0, torch.full_like(e, -118), torch.clamp(e, min=-118))
    return torch.ldexp(torch.ones_like(ref), e - 8)


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound (inf for a non-finite result)."""
    got = got.to(F64)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    if got.numel() == 0:
        return 0.0
    return float(((got - ref).abs() / bound).max())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _levels(P, g):
    """P distinct (scale, offset / scale) pairs: scales 0.25 .. 4 (geometric), offsets 0 and 0.5 .. sqrt(63) standard deviations
    (geometric, so kappa = 1 + t^2 spans 1 .. 64); neighbouring levels differ by > 25 %.  Dealt in a seeded random order."""
    nt = max(2, math.ceil(math.sqrt(1.3 * P)))
    ns = max(2, math.ceil(P / nt))
    scales = 0.25 * 16.0 ** (torch.arange(ns, dtype=F64) / (ns - 1))
    ts = torch.cat([torch.zeros(1, dtype=F64), 0.5 * (math.sqrt(63.0) / 0.5) ** (torch.arange(nt - 1, dtype=F64) / max(nt - 2, 1))])
    perm = torch.randperm(ns * nt, generator=g)[:P]
    return scales[perm // nt], ts[perm % nt] * torch.where(torch.rand(P, generator=g, dtype=F64) < 0.5, -1.0, 1.0)


def _standardised(shape, g):
    """Noise with mean exactly 0 and standard deviation exactly 1 along the last dimension."""
    z = torch.randn(*shape, generator=g, dtype=F64)
    z = z - z.mean(-1, keepdim=True)
    return z / z.pow(2).mean(-1, keepdim=True).sqrt()


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm(+SiLU)
# ---------------------------------------------------------------------------------------------------------------------
def gn_inputs(N, C, H, W, G, silu, seed, with_add=False):
    """x: offset and scale per (image, group); gamma: one sign per group, alternating; beta nonzero;
    dy = noise + 0.7 + 0.8 xhat sign(gamma).  All bf16 values in float64."""
    g = _gen(seed)
    cg, HW = C // G, H * W
    scale, t = _levels(N * G, g)
    z = _standardised((N * G, cg * HW), g)
    x = ((z + t[:, None]) * scale[:, None]).reshape(N, G, cg, HW).reshape(N, C, H, W)
    x = bf16(x)
    sign = torch.where(torch.arange(G) % 2 == 0, 1.0, -1.0).to(F64).repeat_interleave(cg)
    gamma = bf16(sign * (0.5 + torch.rand(C, generator=g, dtype=F64)))
    beta = bf16(0.3 * torch.randn(C, generator=g, dtype=F64) + 0.2)
    xg = x.reshape(N, G, -1)
    mean = xg.mean(-1)
    xhat = ((xg - mean[..., None]) / (xg - mean[..., None]).pow(2).mean(-1, keepdim=True).sqrt()).reshape(N, C, H, W)
    dy = bf16(torch.randn(N, C, H, W, generator=g, dtype=F64) + 0.7 + 0.8 * xhat * sign.view(1, C, 1, 1))
    add = bf16(torch.randn(N, C, H, W, generator=g, dtype=F64)) if with_add else None
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, add=add, G=G, eps=1e-5, silu=silu)


def _gn_group_stats(x, G, eps, div_extra=0):
    N, C = x.shape[:2]
    xg = x.reshape(N, G, -1)
    M = xg.shape[-1]
    mean = xg.sum(-1) / (M + div_extra)
    if div_extra:
        var = (xg * xg).sum(-1) / (M + div_extra) - mean * mean
    else:
        var = (xg - mean[..., None]).pow(2).mean(-1)
    return mean, (var + eps).rsqrt(), (xg * xg).mean(-1) / var, xg.abs().mean(-1)


def _per_channel(v, cg, lookup=None):
    """[N, G] group values -> [N, C, 1, 1]; ``lookup``: 'next' = the last channel of each group reads the next group's value,
    'other' = every channel reads the other image's value."""
    N, G = v.shape
    c = v.repeat_interleave(cg, dim=1).clone()
    if lookup == "next":
        c[:, cg - 1::cg] = v.roll(-1, 1)
    elif lookup == "other":
        c = c.roll(1, 0)
    return c.view(N, G * cg, 1, 1)


def gn_forward(x, gamma, beta, G, eps, silu, div_extra=0, lookup=None, **_):
    N, C = x.shape[:2]
    cg = C // G
    mean, rstd, kappa, absmean = _gn_group_stats(x, G, eps, div_extra)
    mc, rc, kc = _per_channel(mean, cg, lookup), _per_channel(rstd, cg, lookup), _per_channel(kappa, cg)
    gm, bt = gamma.view(1, C, 1, 1), beta.view(1, C, 1, 1)
    z = gm * ((x - mc) * rc) + bt
    y = z * torch.sigmoid(z) if silu else z
    Tz = rc * gm.abs() * (x.abs() + mc.abs()) + bt.abs()
    T = 1.1 * Tz + y.abs() if silu else Tz          # |silu'| <= 1.1; the sigmoid's own two ulps act on y
    return {"y": (y, ulp_bf16(y) + C_GN * kc * T),
            # mean: fp32 result of an fp64 sum of fp32 partial sums
            "mean": (mean, 2.0 ** -24 * mean.abs() + GN_DELTA * absmean),
            "rstd": (rstd, rstd * (0.5 * kappa * GN_DELTA + GN_RSTD_EXTRA))}


def gn_backward(x, gamma, beta, dy, G, eps, silu, add=None, m1_scale=1.0, m2_scale=1.0, div_extra=0, lookup=None,
                sigmoid_for_dsilu=False, **_):
    """dx = rstd (gamma dz - m1 - xhat m2) (+ add), dz = dy silu'(z); the group sums m1 = mean(gamma dz), m2 = mean(gamma dz xhat)."""
    N, C = x.shape[:2]
    cg = C // G
    mean, rstd, kappa, _ = _gn_group_stats(x, G, eps)
    mc, rc, kc = _per_channel(mean, cg, lookup), _per_channel(rstd, cg, lookup), _per_channel(kappa, cg)
    gm, bt = gamma.view(1, C, 1, 1), beta.view(1, C, 1, 1)
    xh = (x - mc) * rc
    if silu:
        z = gm * xh + bt
        sg = torch.sigmoid(z)
        d1 = sg if sigmoid_for_dsilu else sg * (1 + z * (1 - sg))
        # first-order reach of xhat's error into silu'(z): |silu''| <= 1/2, d z = gamma d xhat, d xhat <= c kappa (|xhat| + 1)
        Tdz = (gm * dy).abs() * (d1.abs() + 0.5 * gm.abs() * (xh.abs() + 1))
    else:
        d1 = torch.ones_like(x)
        Tdz = (gm * dy).abs()
    t = gm * dy * d1
    M = cg * x.shape[2] * x.shape[3]
    m1 = t.reshape(N, G, -1).sum(-1) / (M + div_extra) * m1_scale
    m2 = (t * xh).reshape(N, G, -1).sum(-1) / (M + div_extra) * m2_scale
    m1c, m2c = _per_channel(m1, cg, lookup), _per_channel(m2, cg, lookup)
    dx = rc * (t - m1c - xh * m2c)
    T = rc * (Tdz + m1c.abs() + (xh * m2c).abs())
    if add is not None:
        dx = dx + add
        T = T + add.abs()
    T1 = Tdz.reshape(N, G, -1).mean(-1)
    T2 = (Tdz * (xh.abs() + 1)).reshape(N, G, -1).mean(-1)
    props = {"m1_share": float(((m1c.abs() + 0 * t) / t.abs().clamp_min(1e-300)).median()),
             "m2_share": float(((xh * m2c).abs() / t.abs().clamp_min(1e-300)).median())}
    return {"dx": (dx, ulp_bf16(dx) + C_GN * kc * T),
            "m1": (m1, 2.0 ** -23 * m1.abs() + C_GN * kappa * T1),
            "m2": (m2, 2.0 ** -23 * m2.abs() + C_GN * kappa * T2),
            "_props": props}


def groups_differ(mean, rstd, rel=0.1):
    """Every pair of rows of (mean, rstd) differs by at least ``rel`` (of the larger magnitude) in mean or in rstd."""
    m, r = mean.reshape(-1), rstd.reshape(-1)
    dm = (m[:, None] - m[None, :]).abs() >= rel * torch.maximum(m[:, None].abs(), m[None, :].abs())
    dr = (r[:, None] - r[None, :]).abs() >= rel * torch.maximum(r[:, None], r[None, :])
    ok = dm | dr | torch.eye(m.numel(), dtype=torch.bool)
    return bool(ok.all())


# ---------------------------------------------------------------------------------------------------------------------
# add + LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def ln_inputs(rows, C, with_res, seed):
    """s = x + residual with an offset and a scale per row; one weight in eight negative; bias nonzero;
    dy = noise + 0.7 + 0.8 xhat sign(w); ds (the gradient on the residual stream) = noise."""
    g = _gen(seed)
    scale, t = _levels(rows, g)
    s = (_standardised((rows, C), g) + t[:, None]) * scale[:, None]
    if with_res:
        r = bf16(torch.randn(rows, C, generator=g, dtype=F64))
        x = bf16(s - r)
        s = bf16(x + r)
    else:
        r, x = None, bf16(s)
        s = x
    sign = torch.where(torch.arange(C) % 8 == 5, -1.0, 1.0).to(F64)
    w = bf16(sign * (0.5 + torch.rand(C, generator=g, dtype=F64)))
    b = bf16(0.3 * torch.randn(C, generator=g, dtype=F64) + 0.2)
    mean = s.mean(-1, keepdim=True)
    xhat = (s - mean) / (s - mean).pow(2).mean(-1, keepdim=True).sqrt()
    dy = bf16(torch.randn(rows, C, generator=g, dtype=F64) + 0.7 + 0.8 * xhat * sign)
    ds = bf16(torch.randn(rows, C, generator=g, dtype=F64))
    return dict(x=x, r=r, w=w, b=b, dy=dy, ds=ds, eps=1e-5)


def _ln_stats(s, eps, div_extra=0, lookup=None):
    C = s.shape[-1]
    mean = s.sum(-1, keepdim=True) / (C + div_extra)
    var = (s - mean).pow(2).sum(-1, keepdim=True) / (C + div_extra)
    rstd = (var + eps).rsqrt()
    if lookup == "other":
        mean, rstd = mean.roll(1, 0), rstd.roll(1, 0)
    return mean, rstd


def ln_forward(x, r, w, b, eps, div_extra=0, lookup=None, **_):
    s = x if r is None else bf16(x + r)           # the residual stream stays bf16, as in eager
    mean, rstd = _ln_stats(s, eps, div_extra, lookup)
    y = (s - mean) * rstd * w + b
    T = rstd * w.abs() * (s.abs() + mean.abs()) + b.abs()
    return {"s": (s, ulp_bf16(s)), "y": (y, ulp_bf16(y) + C_LN * T)}


def ln_backward(x, r, w, dy, ds, eps, m1_scale=1.0, m2_scale=1.0, div_extra=0, lookup=None, **_):
    """d s = rstd (a - mean(a) - xhat mean(a xhat)) + ds,  a = w dy."""
    s = x if r is None else bf16(x + r)
    C = s.shape[-1]
    mean, rstd = _ln_stats(s, eps, 0, lookup)
    xh = (s - mean) * rstd
    a = w * dy
    m1 = a.sum(-1, keepdim=True) / (C + div_extra) * m1_scale
    m2 = (a * xh).sum(-1, keepdim=True) / (C + div_extra) * m2_scale
    if lookup == "other":
        m1, m2 = m1.roll(1, 0), m2.roll(1, 0)
    dx = rstd * (a - m1 - xh * m2)
    # the recomputed mean errs by 38 u mean|s|, i.e. xhat by 38 u rho with rho = rstd mean|s| (~ sqrt(kappa)): it reaches dx
    # through xhat m2 and through m2 = mean(a xhat) itself
    rho = rstd * s.abs().mean(-1, keepdim=True)
    T = rstd * (a.abs() + m1.abs() + (xh * m2).abs() + rho * (m2.abs() + a.abs().mean(-1, keepdim=True) * xh.abs()))
    if ds is not None:
        dx, T = dx + ds, T + ds.abs()
    props = {"m1_share": float((m1.abs().expand_as(a) / a.abs().clamp_min(1e-300)).median()),
             "m2_share": float(((xh * m2).abs() / a.abs().clamp_min(1e-300)).median())}
    return {"dx": (dx, ulp_bf16(dx) + C_LN * T), "_props": props}


# ---------------------------------------------------------------------------------------------------------------------
# row softmax
# ---------------------------------------------------------------------------------------------------------------------
def softmax_inputs(rows, L, seed):
    """Rows of very different temperature, a row of equal values, a row with one finite-looking entry; dp = noise + 1."""
    g = _gen(seed)
    x = torch.randn(rows, L, generator=g, dtype=F64) * torch.logspace(-1, 1.3, rows, dtype=F64)[:, None]
    x[0] = 3.0
    if L > 8:
        x[1, 1:] = -30000.0
    dp = bf16(torch.randn(rows, L, generator=g, dtype=F64) + 1.0)
    return dict(x=bf16(x), dp=dp)


def softmax_forward(x, extra=False, lookup=None, **_):
    m = x.max(-1, keepdim=True).values
    e = torch.exp(x - m)
    den = e.sum(-1, keepdim=True) + (1.0 if extra else 0.0)        # extra: the row's maximum (e = 1) summed twice
    if lookup == "other":
        den = den.roll(1, 0)
    p = e / den
    T = p * (1 + (x.abs() + m.abs()) / 64)
    return {"p": (p, ulp_bf16(p) + C_SOFTMAX * T)}


def softmax_backward(p, dp, dot_scale=1.0, extra=False, lookup=None, **_):
    """ds = p (dp - sum(p dp)) on the GIVEN bf16 probabilities (the kernel's input)."""
    dot = (p * dp).sum(-1, keepdim=True)
    if extra:                                                       # the element of the largest p summed twice
        dot = dot + (p * dp).gather(-1, p.argmax(-1, keepdim=True))
    dot = dot * dot_scale
    if lookup == "other":
        dot = dot.roll(1, 0)
    ds = p * (dp - dot)
    T = p.abs() * (dp.abs() + dot.abs() + (p * dp).abs().sum(-1, keepdim=True))
    props = {"dot_share": float((dot.abs().expand_as(dp) / dp.abs().clamp_min(1e-300)).median())}
    return {"ds": (ds, ulp_bf16(ds) + C_SOFTMAX * T), "_props": props}


# ---------------------------------------------------------------------------------------------------------------------
# attention, head dim 64, scale 1/8
# ---------------------------------------------------------------------------------------------------------------------
ATTN_HEAD_SCALES = (0.5, 0.9, 1.3)       # logits q k / 8 ~ N(0, scale^2): inside the +-6 the iid tests of test_nn_gpu.py reach


def attention_inputs(B, H, S, Skv, seed, zero_q=False):
    """q ~ N(0, 1) times a temperature per head (or all zero); k, v ~ N(0, 1) + 0.5: with the common offset neither
    D = rowsum(dO o O) nor the P-weighted mean of the keys that multiplies it in dq averages out over a diffuse row (the
    offset moves all logits of a query together, so the probabilities are those of the centred keys);
    dO = noise + 3 O + 0.5.  [B, S, H, 64] / [B, Skv, H, 64]."""
    g = _gen(seed)
    hs = torch.tensor([ATTN_HEAD_SCALES[h % len(ATTN_HEAD_SCALES)] for h in range(H)], dtype=F64).view(1, 1, H, 1)
    q = bf16(torch.randn(B, S, H, 64, generator=g, dtype=F64) * hs)
    if zero_q:
        q = torch.zeros_like(q)
    k = bf16(torch.randn(B, Skv, H, 64, generator=g, dtype=F64) + 0.5)
    v = bf16(torch.randn(B, Skv, H, 64, generator=g, dtype=F64) + 0.5)
    o = attention_forward(q, k, v)["o"][0]
    do = bf16(torch.randn(B, S, H, 64, generator=g, dtype=F64) + 3.0 * o + 0.5)
    return dict(q=q, k=k, v=v, do=do)


def _attn_probs(q, k, extra_key):
    if extra_key:                   # one key past Skv admitted with score 0 (a zero row, as the padded tile holds)
        k = torch.cat([k, torch.zeros_like(k[:, :1])], 1)
    sc = torch.einsum("bshd,bthd->bhst", q, k) / 8.0
    lse = torch.logsumexp(sc, -1)
    return sc, lse, torch.exp(sc - lse[..., None]), k


def attention_forward(q, k, v, extra_key=False, **_):
    """o [B, S, H, 64] and the log-sum-exp [B, H, S] of the scaled scores."""
    sc, lse, P, k2 = _attn_probs(q, k, extra_key)
    if extra_key:
        v = torch.cat([v, torch.zeros_like(v[:, :1])], 1)
    o = torch.einsum("bhst,bthd->bshd", P, v)
    T = torch.einsum("bhst,bthd->bshd", P, v.abs())
    A = torch.einsum("bshd,bthd->bhst", q.abs(), k2.abs()).max(-1).values / 8.0
    Skv = k2.shape[1]
    lse_bound = C_LSE_SCORE * A + 2.0 ** -22 * (lse.abs() + sc.max(-1).values.abs()) + (Skv + 64) * 2.0 ** -24 + 2.0 ** -21
    return {"o": (o, ulp_bf16(o) + C_ATTN * T), "lse": (lse, lse_bound)}


def attention(q, k, v, do, o_saved=None, d_scale=1.0, extra_key=False, **_):
    """The training node as one operation: o, lse, dq, dk, dv."""
    out = attention_forward(q, k, v, extra_key=extra_key)
    out.update(attention_backward(q, k, v, do, o_saved=o_saved, d_scale=d_scale, extra_key=extra_key))
    return out


def attention_backward(q, k, v, do, o_saved=None, d_scale=1.0, extra_key=False, **_):
    """dq, dk, dv.  ``o_saved``: the bf16 output the node kept; D = rowsum(dO o O) is formed from it, as every flash backward
    does (default: the float64 output rounded to bf16)."""
    Skv = k.shape[1]
    sc, lse, P, k2 = _attn_probs(q, k, extra_key)
    v2 = torch.cat([v, torch.zeros_like(v[:, :1])], 1) if extra_key else v
    if o_saved is None:
        o_saved = bf16(torch.einsum("bhst,bthd->bshd", P, v2))
    D = torch.einsum("bshd,bshd->bhs", do, o_saved) * d_scale
    dP = torch.einsum("bshd,bthd->bhst", do, v2)
    dS = P * (dP - D[..., None])
    # magnitude of dP - D before it cancels (fp32 sums of 64 products each)
    A = torch.einsum("bshd,bthd->bhst", do.abs(), v2.abs()) + torch.einsum("bshd,bshd->bhs", do.abs(), o_saved.abs())[..., None]
    PA = P * A
    dq = torch.einsum("bhst,bthd->bshd", dS, k2) / 8.0
    dk = torch.einsum("bhst,bshd->bthd", dS, q) / 8.0
    dv = torch.einsum("bhst,bshd->bthd", P, do)
    Tq = torch.einsum("bhst,bthd->bshd", dS.abs(), k2.abs()) / 8.0
    Tk = torch.einsum("bhst,bshd->bthd", dS.abs(), q.abs()) / 8.0
    Tv = torch.einsum("bhst,bshd->bthd", P, do.abs())
    Tq2 = torch.einsum("bhst,bthd->bshd", PA, k2.abs()) / 8.0
    Tk2 = torch.einsum("bhst,bshd->bthd", PA, q.abs()) / 8.0
    props = {"D_share": float((D.abs()[..., None].expand_as(dP) / dP.abs().clamp_min(1e-300)).median())}
    cut = lambda t: t[:, :Skv]      # noqa: E731
    return {"dq": (dq, ulp_bf16(dq) + C_ATTN * Tq + C_ATTN_FP32 * Tq2),
            "dk": (cut(dk), ulp_bf16(cut(dk)) + C_ATTN * cut(Tk) + C_ATTN_FP32 * cut(Tk2)),
            "dv": (cut(dv), ulp_bf16(cut(dv)) + C_ATTN * cut(Tv)),
            "_props": props}


# ---------------------------------------------------------------------------------------------------------------------
# wrong formulas: name -> keyword arguments of the reference function of ``op``.  ``None`` marks one that does not apply to a
# case (a single image has no other image; SiLU off has no silu').
# ---------------------------------------------------------------------------------------------------------------------
def _gn_div(case):
    return {"div_extra": case["x"].shape[1] // case["G"]}


MUTANTS = {
    "gn_forward": [
        ("divisor M + C/G", _gn_div),
        ("next group's statistics on a group's last channel", lambda c: {"lookup": "next"}),
        ("the other image's statistics", lambda c: {"lookup": "other"} if c["x"].shape[0] > 1 else None),
    ],
    "gn_backward": [
        ("m1 x 0.95", lambda c: {"m1_scale": 0.95}),
        ("m2 x 0.95", lambda c: {"m2_scale": 0.95}),
        ("divisor M + C/G", _gn_div),
        ("next group's statistics on a group's last channel", lambda c: {"lookup": "next"}),
        ("the other image's statistics", lambda c: {"lookup": "other"} if c["x"].shape[0] > 1 else None),
        ("silu' replaced by sigmoid", lambda c: {"sigmoid_for_dsilu": True} if c["silu"] else None),
    ],
    "ln_forward": [
        ("divisor C + 1", lambda c: {"div_extra": 1}),
        ("the other row's statistics", lambda c: {"lookup": "other"}),
    ],
    "ln_backward": [
        ("m1 x 0.95", lambda c: {"m1_scale": 0.95}),
        ("m2 x 0.95", lambda c: {"m2_scale": 0.95}),
        ("divisor C + 1", lambda c: {"div_extra": 1}),
        ("the other row's statistics", lambda c: {"lookup": "other"}),
    ],
    "softmax_forward": [
        ("one row element more in the sum (the maximum twice)", lambda c: {"extra": True}),
        ("the other row's sum", lambda c: {"lookup": "other"}),
    ],
    "softmax_backward": [
        ("dot x 0.95", lambda c: {"dot_scale": 0.95}),
        ("one row element more in the dot (the largest p twice)", lambda c: {"extra": True}),
        ("the other row's dot", lambda c: {"lookup": "other"}),
    ],
    # one node, five outputs: a key admitted past Skv renormalises every probability, which the LSE shows first
    "attention": [
        ("D x 0.95", lambda c: {"d_scale": 0.95}),
        ("one key past Skv admitted with score 0", lambda c: {"extra_key": True}),
    ],
}

REFERENCES = {"gn_forward": gn_forward, "gn_backward": gn_backward, "ln_forward": ln_forward, "ln_backward": ln_backward,
              "softmax_forward": softmax_forward, "softmax_backward": softmax_backward,
              "attention_forward": attention_forward, "attention_backward": attention_backward, "attention": attention}


def call(op, case, **mutation):
    """The reference of ``op`` on a case's inputs (a dict from the ``*_inputs`` functions), optionally mutated."""
    args = {k: v for k, v in case.items()}
    args.update(mutation)
    return REFERENCES[op](**args)


def tensors(result):
    return {k: v for k, v in result.items() if not k.startswith("_")}
