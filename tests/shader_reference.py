"""The neural shader and the shading loss of the deformer's second stage (the reference's deformer/modules/neuralshader.py
and deformer/losses/shading.py; the definition with its rounding points: DESIGN.md section 3.25) in torch on the CPU, by
dtype, in two forms.

UNROUNDED: the plain network (positional encoding, five ``diffuse`` and three ``specular`` linears, ReLU, sigmoid) and the
shading loss in the dtype of its inputs, differentiated by autograd: what the reference computes, as a masked sum and as the
reference's boolean gather.

ROUNDED: the same with the rounding points of include/gd_shader.h -- features, weights, every activation, ``dlogits`` and
every masked ``dX`` to bf16 (round to nearest even), products accumulated and everything else kept in the ACCUMULATION dtype (float32 as
such a kernel, or float64) -- with the backward written out, because its rounding points are not autograd's.

A case is a dict of mesh_losses_reference.make_case plus ``rgb`` [H,W,3]; parameters are a dict under the reference's names
(``diffuse.network.{0..4}.linear.{weight,bias}``, ``specular.network.{0..2}.linear.{weight,bias}``)."""
import numpy as np
import torch

from tests import mesh_losses_reference as lref

IN_FEATURES = (27, 256, 256, 256, 256, 262, 128, 128)
OUT_FEATURES = (256, 256, 256, 256, 256, 128, 128, 3)
RELU = (True, True, True, True, False, True, True, False)
NAMES = [f"diffuse.network.{i}.linear" for i in range(5)] + [f"specular.network.{i}.linear" for i in range(3)]
FREQUENCIES = (1.0, 2.0, 4.0, 8.0)
NORM_EPS = 1e-12


def make_params(seed):
    """Seeded float32 parameters: weights normal x sqrt(2 / fan_in), biases uniform in +-0.5 (zero biases, the shader's own
    initialisation, would leave the bias path untested).  Drawn layer by layer, weight then bias."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, k, o in zip(NAMES, IN_FEATURES, OUT_FEATURES):
        out[name + ".weight"] = (rng.normal(size=(o, k)) * np.sqrt(2.0 / k)).astype(np.float32)
        out[name + ".bias"] = rng.uniform(-0.5, 0.5, o).astype(np.float32)
    return out


def make_rgb(H, W, seed):
    return np.random.RandomState(seed).uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)


# the golden views of tests/golden/shader_pins.npz: what tests/golden/make_golden_shader.py feeds the reference's own code
GOLDEN_SEED = 7                                                              # of make_params
GOLDEN_CASES = {"view0": (9, 11, 101, 201), "view1": (16, 16, 102, 202)}     # H, W, the case's seed, the seed of rgb
GOLDEN_INPUT_KEYS = ("normal", "position", "mask", "tmask", "R", "center", "rgb")


def golden_cases():
    return {name: dict(lref.make_case(H, W, seed), rgb=make_rgb(H, W, rgb_seed))
            for name, (H, W, seed, rgb_seed) in GOLDEN_CASES.items()}


def param_tensors(params, dtype):
    """(weights, biases): two lists of eight leaves in ``dtype``"""
    ws = [torch.from_numpy(params[n + ".weight"]).to(dtype).requires_grad_(True) for n in NAMES]
    bs = [torch.from_numpy(params[n + ".bias"]).to(dtype).requires_grad_(True) for n in NAMES]
    return ws, bs


# ---- selection ---------------------------------------------------------------------------------------------------------

def hash32(seed, step, index):
    """``gd_shader_hash32`` of include/gd_shader.h, bit for bit, on uint32 arrays: a valid pixel is kept when this is below
    ``keep_threshold(p)``."""
    with np.errstate(over="ignore"):
        x = np.asarray(index, dtype=np.uint32) ^ (np.uint32(seed) * np.uint32(0x9E3779B1)) ^ (np.uint32(step) * np.uint32(0x85EBCA77))
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846CA68B)
        x = x ^ (x >> np.uint32(16))
    return x


def valid_pixels(case, dtype):
    """bool [H W]: view mask > 0, G-buffer mask > 0 and cos_1e-6(d, n_cam) <= 0"""
    c = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dtype) for k in ("position", "normal", "mask", "tmask", "R", "center")}
    with torch.no_grad():
        cv = lref.cosine(lref.view_direction(c["position"], c["R"], c["center"]), lref.to_camera(c["normal"], c["R"]), lref.VIEW_EPS)
        return ((c["tmask"][..., 0] > 0) & (c["mask"][..., 0] > 0) & (cv <= 0)).reshape(-1).numpy()


def keep_threshold(p):
    """``gd_shader_keep_threshold``: floor(p 2^32) of the float32 ``p``, 0 <= p < 1"""
    return np.uint32(int(np.floor(float(np.float32(p)) * 4294967296.0)))


def packed_offset(l):
    """``gd_shader_packed_offset``: the first half of W_l, [Op_l][Kp_l], in the packed weights"""
    pad = lambda n: (n + 31) // 32 * 32
    return sum(pad(OUT_FEATURES[i]) * (pad(IN_FEATURES[i]) if i != 5 else 288) for i in range(l))


def kept_pixels(case, dtype, p=1.0, seed=0, step=0):
    """bool [H W]: the valid pixels whose hash is below floor(p 2^32); all of them when p >= 1"""
    valid = valid_pixels(case, dtype)
    if p >= 1:
        return valid
    return valid & (hash32(seed, step, np.arange(valid.shape[0])) < keep_threshold(p))


# ---- features ----------------------------------------------------------------------------------------------------------

def encode(p):
    return torch.cat([p] + [fn(p * f) for f in FREQUENCIES for fn in (torch.sin, torch.cos)], dim=-1)


def view_dir(position, center):
    v = center - position
    return v / v.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS)


# ---- unrounded ---------------------------------------------------------------------------------------------------------

def network(ws, bs, position, normal, direction):
    """colour [..., 3] of the plain network in the dtype of its arguments"""
    h = encode(position)
    for l in range(5):
        h = h @ ws[l].T + bs[l]
        if RELU[l]:
            h = torch.relu(h)
    h = torch.cat([h, normal, direction], dim=-1)
    for l in range(5, 8):
        h = h @ ws[l].T + bs[l]
        if RELU[l]:
            h = torch.relu(h)
    return torch.sigmoid(h)


def _inputs(case, dtype):
    position = torch.from_numpy(case["position"]).to(dtype).reshape(-1, 3).requires_grad_(True)
    normal = torch.from_numpy(case["normal"]).to(dtype).reshape(-1, 3).requires_grad_(True)
    center = torch.from_numpy(case["center"]).to(dtype)
    rgb = torch.from_numpy(case["rgb"]).to(dtype).reshape(-1, 3)
    return position, normal, center, rgb


def _result(case, loss, colour, position, normal, ws, bs, keep):
    if loss.requires_grad:
        loss.backward()
    shape = case["position"].shape
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    full = np.zeros((keep.shape[0], 3), dtype=np.float64)
    full[keep] = colour.detach().numpy()
    return {"loss": float(loss.detach()), "colour": full.reshape(shape), "kept": keep,
            "dposition": zero(position).numpy().reshape(shape), "dnormal": zero(normal).numpy().reshape(shape),
            "dW": [zero(w).numpy() for w in ws], "db": [zero(b).numpy() for b in bs]}


def unrounded(case, params, dtype, keep, gather=True):
    """The loss of one view over the pixels ``keep`` (bool [H W]) and its gradients, in ``dtype``.  ``gather=True``: the
    reference's form (``x[keep]`` first); ``False``: the masked-sum form (every pixel is shaded, a pixel that is out adds 0)."""
    position, normal, center, rgb = _inputs(case, dtype)
    ws, bs = param_tensors(params, dtype)
    k = torch.from_numpy(keep)
    count = int(keep.sum())
    if gather:
        p, n = position[k], normal[k]
        colour = network(ws, bs, p, n, torch.nn.functional.normalize(center - p, dim=-1))
        loss = torch.nn.functional.l1_loss(colour, rgb[k]) if count else colour.sum() * 0
    else:
        every = network(ws, bs, position, normal, view_dir(position, center))
        terms = torch.where(k[:, None], (every - rgb).abs(), torch.zeros_like(every))
        loss = terms.sum() / (3 * count) if count else terms.sum() * 0
        colour = every[k]
    return _result(case, loss, colour, position, normal, ws, bs, keep)


# ---- rounded -----------------------------------------------------------------------------------------------------------

def bf16(x):
    """round to nearest even to bf16, kept in the dtype of ``x``"""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def rounded_mlp(ws, bs, feat, extra, dlogits_of):
    """The eight products with the kernels' rounding points in the dtype of ``ws`` (the accumulation dtype).  ``feat`` [N,27]
    and ``extra`` [N,6] unrounded; ``dlogits_of(logits)`` gives the gradient towards the logits.  Returns (logits, dfeat,
    dextra, dW, db, activations, dZ)."""
    wq = [bf16(w) for w in ws]
    X = [bf16(feat)]
    for l in range(8):
        if l == 5:
            X[5] = torch.cat([X[5], bf16(extra)], dim=-1)
        z = X[l] @ wq[l].T + bs[l]
        if l == 7:
            logits = z
        else:
            X.append(bf16(torch.relu(z) if RELU[l] else z))
    dZ = [None] * 8
    dZ[7] = bf16(dlogits_of(logits))
    dW, db = [None] * 8, [None] * 8
    dfeat = dextra = None
    for l in range(7, -1, -1):
        dW[l] = dZ[l].T @ X[l]
        db[l] = dZ[l].sum(0)
        dX = dZ[l] @ wq[l]
        if l == 0:
            dfeat = dX
        elif l == 5:
            dextra = dX[:, 256:]
            dZ[4] = bf16(dX[:, :256])
        else:
            dZ[l - 1] = bf16(torch.where(X[l] > 0, dX, torch.zeros_like(dX)) if RELU[l - 1] else dX)
    return logits, dfeat, dextra, dW, db, X, dZ


def rounded(case, params, acc_dtype, keep):
    """The rounded statement of one view over the pixels ``keep``: same keys as ``unrounded``."""
    with torch.no_grad():
        position, normal, center, rgb = (t.detach() for t in _inputs(case, acc_dtype))
        ws, bs = (list(t.detach() for t in ts) for ts in param_tensors(params, acc_dtype))
        k = torch.from_numpy(keep)
        count = int(keep.sum())
        p, n, target = position[k], normal[k], rgb[k]
        v = center - p
        length = v.norm(dim=-1, keepdim=True)
        u = v / length.clamp_min(NORM_EPS)
        out = {}

        def dlogits_of(logits):
            c = torch.sigmoid(logits)
            out["colour"] = c
            out["loss"] = (c - target).abs().sum() / (3 * count) if count else c.sum() * 0
            return torch.sign(c - target) * (c * (1 - c)) / (3 * count) if count else torch.zeros_like(c)

        _, dfeat, dextra, dW, db, _, _ = rounded_mlp(ws, bs, encode(p), torch.cat([n, u], dim=-1), dlogits_of)
        dp = dfeat[:, :3].clone()
        for j, f in enumerate(FREQUENCIES):
            dp = dp + f * (torch.cos(f * p) * dfeat[:, 3 + 6 * j:6 + 6 * j] - torch.sin(f * p) * dfeat[:, 6 + 6 * j:9 + 6 * j])
        gu = dextra[:, 3:6]
        gv = torch.where(length > NORM_EPS, (gu - u * (u * gu).sum(-1, keepdim=True)) / length.clamp_min(NORM_EPS), gu / NORM_EPS)
        shape = case["position"].shape
        dposition = torch.zeros_like(position)
        dnormal = torch.zeros_like(normal)
        dposition[k] = dp - gv
        dnormal[k] = dextra[:, :3]
        full = np.zeros((keep.shape[0], 3), dtype=np.float64)
        full[keep] = out["colour"].numpy()
        return {"loss": float(out["loss"]), "colour": full.reshape(shape), "kept": keep,
                "dposition": dposition.numpy().reshape(shape), "dnormal": dnormal.numpy().reshape(shape),
                "dW": [w[:o, :i].numpy() for w, o, i in zip(dW, OUT_FEATURES, IN_FEATURES)], "db": [b.numpy() for b in db]}


def l1_signs(result, case):
    """sign(colour - rgb) at the kept pixels: what must agree between two statements for their gradients to be comparable"""
    return np.sign(result["colour"].reshape(-1, 3)[result["kept"]] - case["rgb"].reshape(-1, 3)[result["kept"]].astype(np.float64))


def normalised_error(g, g64):
    """max |g - g64| / max |g64| (0 / 0 = 0)"""
    g64 = np.asarray(g64, dtype=np.float64)
    top = np.abs(g64).max() if g64.size else 0.0
    err = np.abs(np.asarray(g, dtype=np.float64) - g64).max() if g64.size else 0.0
    return float(err / top) if top > 0 else float(err)


# ---- exact integers ------------------------------------------------------------------------------------------------------

def _selection(l):
    """Layer ``l`` as a selection matrix: output o copies one input (layer 5 reaches into ``extra``; layer 7 adds three)."""
    k, o = IN_FEATURES[l], OUT_FEATURES[l]
    w = np.zeros((o, k))
    if l == 7:
        for c in range(3):
            w[c, c] = w[c, 122 + c] = w[c, 125 + c] = 1      # the last two trace back to ``normal`` and ``view_dir``
    elif l == 5:
        w[np.arange(o), 134 + np.arange(o)] = 1
    else:
        w[np.arange(o), np.arange(o) % k] = 1
    return w


def exact_case(dense, n, seed):
    """Small-integer inputs in the manner of tests/exact_reference.py: every value the kernels round to bf16 is an integer of
    magnitude <= 256 (asserted in tests/test_shader_cpu.py), so each result of a kernel has ONE bit pattern.  Layer ``dense`` holds a
    matrix of -1 / 0 / +1 with 60% nonzero entries -- its forward product is a real reduction, more than a third of whose
    products are nonzero -- and the other layers are selection matrices that pass the non-negative integers through the
    ReLUs.  Biases are -1 / 0 / +1, features 0 / 1 / 2, ``extra`` and ``dlogits`` -2 .. 2.  float64 arrays."""
    rng = np.random.RandomState(seed)
    ws, bs = [], []
    for l in range(8):
        k, o = IN_FEATURES[l], OUT_FEATURES[l]
        ws.append(rng.choice([-1.0, 1.0], (o, k)) * (rng.uniform(size=(o, k)) < 0.6) if l == dense else _selection(l))
        bs.append(rng.randint(-1, 2, o).astype(np.float64))
    return {"ws": ws, "bs": bs, "feat": rng.randint(0, 3, (n, 27)).astype(np.float64),
            "extra": rng.randint(-2, 3, (n, 6)).astype(np.float64), "dlogits": rng.randint(-2, 3, (n, 3)).astype(np.float64)}


def exact_expected(case):
    """(logits, dfeat, dextra, dW, db, X, dZ) of ``exact_case`` by the rounded statement in float64 (no rounding happens)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    dlogits = t(case["dlogits"])
    return rounded_mlp([t(w) for w in case["ws"]], [t(b) for b in case["bs"]], t(case["feat"]), t(case["extra"]),
                       lambda logits: dlogits)
