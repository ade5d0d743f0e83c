"""The definitions of include/gd_mesh_losses.h in torch on the CPU, in the dtype of their inputs, in two forms: the
masked-sum form the kernels use (every pixel computes its term, a pixel that is out adds 0) and the boolean-gather form
of the reference (``x[mask]``, ``cosine_similarity``, the sign written into ``.data``).  Plus the seeded generator of
synthetic G-buffers that keeps every threshold of the terms away from the inputs.

A case is a dict of arrays: ``normal``, ``position`` [H,W,3], ``mask`` [H,W,1], the same with ``_rf``, ``T`` [H,W,3] (the
view's normal map in [0,1]), ``tmask`` [H,W,1], ``R`` [3,3], ``center`` [3]."""
import numpy as np
import torch

EPSILON = float(np.float32(-0.1))     # the reference's default, as the float32 the kernel receives
NORM_EPS = 1e-12
ERR_EPS = 1e-8
VIEW_EPS = 1e-6
KEYS = ("normal", "position", "mask", "normal_rf", "position_rf", "mask_rf", "T", "tmask", "R", "center")


def tensors(case, dtype):
    return {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dtype) for k in KEYS}


def _rf(like):
    return torch.diag(torch.tensor([1.0, -1.0, -1.0], dtype=like.dtype, device=like.device))


def to_camera(n, R):
    return n @ R.T @ _rf(n)


def view_direction(p, R, center):
    v = center - p
    u = v / v.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS)
    return -(u @ R.T @ _rf(p))


def cosine(a, b, eps):
    return (a * b).sum(-1) / (a.norm(dim=-1).clamp_min(eps) * b.norm(dim=-1).clamp_min(eps))


def _sign(c):
    return torch.where(c < 0, -torch.ones_like(c), torch.ones_like(c))


# ---- the masked-sum form ---------------------------------------------------------------------------------------------------

def enhanced_parts(c, epsilon=EPSILON):
    """(terms [H W], w [H W], in [H W]): the loss is terms.sum() / w.sum()."""
    n_cam = to_camera(c["normal"], c["R"])
    t = 2 * c["T"] - 1
    e = 1 - cosine(t, n_cam, ERR_EPS)
    with torch.no_grad():
        d = view_direction(c["position"], c["R"], c["center"])
        ct = cosine(d, t, VIEW_EPS)
        ct = torch.where(ct > epsilon, torch.zeros_like(ct), ct)
        cv = cosine(d, n_cam, VIEW_EPS)
        w = torch.exp(ct.abs())
        inside = (c["tmask"][..., 0] > 0) & (c["mask"][..., 0] > 0) & (cv <= 0) & (ct <= epsilon)
    return torch.where(inside, e * w, torch.zeros_like(e)).reshape(-1), w.reshape(-1), inside.reshape(-1)


def enhanced(c, epsilon=EPSILON):
    terms, w, _ = enhanced_parts(c, epsilon)
    return terms.sum() / w.sum()


def plain_parts(c):
    """(terms [H W], in [H W]): the loss is terms.sum() / (3 count)."""
    diff = 0.5 * (to_camera(c["normal"], c["R"]) + 1) - c["T"]
    inside = (c["tmask"][..., 0] > 0) & (c["mask"][..., 0] > 0)
    terms = diff.abs().sum(-1)
    return torch.where(inside, terms, torch.zeros_like(terms)).reshape(-1), inside.reshape(-1)


def plain(c):
    terms, inside = plain_parts(c)
    count = int(inside.sum())
    return terms.sum() / (3 * count) if count else terms.sum() * 0


def hole_signs(c):
    """(s, s_rf, the cosine s stands for): s carries the cosine's gradient and the sign's value."""
    cv = cosine(view_direction(c["position"], c["R"], c["center"]), to_camera(c["normal"], c["R"]), VIEW_EPS)
    with torch.no_grad():
        cv_rf = cosine(view_direction(c["position_rf"], c["R"], c["center"]), to_camera(c["normal_rf"], c["R"]), VIEW_EPS)
    return _sign(cv.detach()) + (cv - cv.detach()), _sign(cv_rf), cv


def hole_parts(c):
    """(terms [H W], in [H W]): the loss is terms.sum() / count."""
    s, s_rf, _ = hole_signs(c)
    inside = (c["mask"][..., 0] > 0) & (c["mask_rf"][..., 0] > 0)
    terms = (s - s_rf) ** 2
    return torch.where(inside, terms, torch.zeros_like(terms)).reshape(-1), inside.reshape(-1)


def hole(c):
    terms, inside = hole_parts(c)
    count = int(inside.sum())
    return terms.sum() / count if count else terms.sum() * 0


LOSSES = {"enhanced": enhanced, "plain": plain, "hole": hole}


# ---- the boolean-gather form -------------------------------------------------------------------------------------------------

def _cos(a, b, eps):
    return torch.nn.functional.cosine_similarity(a, b, dim=-1, eps=eps)


def _direction_gather(p, R, center):
    return torch.nn.functional.normalize(center - p, dim=-1) @ R.T @ _rf(p) * -1


def enhanced_gather(c, epsilon=EPSILON):
    n_cam = to_camera(c["normal"], c["R"])
    t = c["T"] * 2 - 1
    errors = 1 - _cos(t, n_cam, ERR_EPS)
    with torch.no_grad():
        d = _direction_gather(c["position"], c["R"], c["center"])
        ct = _cos(d, t, VIEW_EPS)
        ct[ct > epsilon] = 0
        cv = _cos(d, n_cam, VIEW_EPS)
    weight = torch.exp(ct.abs())
    errors = errors * weight / weight.sum()
    keep = (c["tmask"].squeeze(-1) > 0) & (c["mask"].squeeze(-1) > 0) & (cv <= 0) & (ct <= epsilon)
    return errors[keep].sum()


def plain_gather(c):
    keep = ((c["tmask"] > 0) & (c["mask"] > 0)).squeeze(-1)
    return torch.nn.functional.l1_loss((0.5 * (to_camera(c["normal"], c["R"]) + 1))[keep], c["T"][keep])


def hole_gather(c):
    cv = _cos(_direction_gather(c["position"], c["R"], c["center"]), to_camera(c["normal"], c["R"]), VIEW_EPS)
    cv_rf = _cos(_direction_gather(c["position_rf"], c["R"], c["center"]), to_camera(c["normal_rf"], c["R"]), VIEW_EPS)
    for x in (cv, cv_rf):                      # the value becomes the sign, the graph stays the cosine's
        negative = x.detach() < 0
        x.data[negative] = -1
        x.data[~negative] = 1
    keep = (c["mask"].squeeze(-1) > 0) & (c["mask_rf"].squeeze(-1) > 0)
    return torch.nn.functional.mse_loss(cv[keep], cv_rf[keep])


GATHER_LOSSES = {"enhanced": enhanced_gather, "plain": plain_gather, "hole": hole_gather}


def gradients(case, dtype, fn):
    """(loss, d/dnormal, d/dposition) of ``fn`` on ``case`` in ``dtype`` as numpy; a gradient autograd does not produce is 0."""
    c = tensors(case, dtype)
    c["normal"].requires_grad_(True)
    c["position"].requires_grad_(True)
    loss = fn(c)
    if loss.requires_grad:
        loss.backward()
    out = [loss.detach().numpy()]
    for k in ("normal", "position"):
        out.append(np.zeros(case[k].shape, dtype=out[0].dtype) if c[k].grad is None else c[k].grad.numpy())
    return tuple(out)


def selections(case, dtype, epsilon=EPSILON):
    """What a dtype decides at the thresholds: the three pixel sets, the two facing signs and the signs of the L1 term."""
    with torch.no_grad():
        c = tensors(case, dtype)
        s, s_rf, _ = hole_signs(c)
        diff = 0.5 * (to_camera(c["normal"], c["R"]) + 1) - c["T"]
        return {"enhanced": enhanced_parts(c, epsilon)[2].numpy(), "plain": plain_parts(c)[1].numpy(),
                "hole": hole_parts(c)[1].numpy(), "s": s.numpy(), "s_rf": s_rf.numpy(), "l1": torch.sign(diff).numpy()}


# ---- synthetic G-buffers ----------------------------------------------------------------------------------------------------

MARGIN = 1e-3


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _draw(rng, n, R, center):
    """``n`` pixels: normals of length 0.6 .. 1 that mostly face the camera, positions in a unit box, a normal map near the
    normal, a reference mesh near the mesh that faces the other way at a third of the pixels."""
    position = rng.uniform(-0.5, 0.5, (n, 3))
    normal = _unit(rng.normal(size=(n, 3)))
    toward = _unit(center - position)
    away = (normal * toward).sum(-1) < 0
    flip = away & (rng.uniform(size=n) < 0.8)
    normal[flip] *= -1
    n_cam = (normal @ R.T) * np.array([1.0, -1.0, -1.0])
    T = 0.5 * (_unit(n_cam + 0.4 * rng.normal(size=(n, 3))) + 1)
    normal_rf = _unit(normal + 0.2 * rng.normal(size=(n, 3))) * np.where(rng.uniform(size=n) < 0.35, -1.0, 1.0)[:, None]
    position_rf = position + 0.02 * rng.normal(size=(n, 3))
    normal = normal * rng.uniform(0.6, 1.0, (n, 1))
    return [a.astype(np.float32) for a in (normal, position, normal_rf, position_rf, T)]


def _near_a_threshold(case):
    c = tensors(case, torch.float64)
    with torch.no_grad():
        n_cam, t = to_camera(c["normal"], c["R"]), 2 * c["T"] - 1
        d = view_direction(c["position"], c["R"], c["center"])
        cv = cosine(d, n_cam, VIEW_EPS)
        cv_rf = cosine(view_direction(c["position_rf"], c["R"], c["center"]), to_camera(c["normal_rf"], c["R"]), VIEW_EPS)
        ct = cosine(d, t, VIEW_EPS) - EPSILON
        diff = (0.5 * (n_cam + 1) - c["T"]).abs().min(-1).values
        near = (cv.abs() < MARGIN) | (cv_rf.abs() < MARGIN) | (ct.abs() < MARGIN) | (diff < MARGIN)
    return near.numpy()


def make_case(H, W, seed):
    """A seeded case of H x W pixels.  Masks are exactly 0 (a fifth of the pixels each) or in [0.05, 1].  Every pixel whose
    float64 cv, cv_rf, ct - epsilon or 0.5 (n_cam + 1) - T lies within ``MARGIN`` of zero is drawn again until none is
    left, and the whole image is drawn again until every term has a pixel that is in and the hole term is not 0."""
    rng = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    R = (q * np.sign(np.linalg.det(q))).astype(np.float32)
    center = (np.array([0.3, -0.2, 3.0]) + 0.1 * rng.normal(size=3)).astype(np.float32)
    n = H * W
    names = ("normal", "position", "normal_rf", "position_rf", "T")
    for _ in range(1000):
        case = {"R": R, "center": center}
        for k, a in zip(names, _draw(rng, n, R.astype(np.float64), center.astype(np.float64))):
            case[k] = a.reshape(H, W, 3)
        for k in ("mask", "mask_rf", "tmask"):
            m = rng.uniform(0.05, 1.0, n) * (rng.uniform(size=n) >= 0.2)
            case[k] = m.astype(np.float32).reshape(H, W, 1)
        while True:
            near = _near_a_threshold(case).reshape(-1)
            if not near.any():
                break
            for k, a in zip(names, _draw(rng, int(near.sum()), R.astype(np.float64), center.astype(np.float64))):
                case[k].reshape(n, 3)[near] = a
        sel = selections(case, torch.float64)
        if sel["enhanced"].any() and sel["plain"].any() and (sel["hole"].reshape(-1) & (sel["s"] != sel["s_rf"]).reshape(-1)).any():
            return case
    raise RuntimeError("make_case: no image with every term present")


def scalar_sums(terms):
    """torch's sum, the ascending and the descending sequential sum of one array of terms (mesh_geometry_reference)."""
    return [terms.sum(), torch.cumsum(terms, 0)[-1], torch.cumsum(terms.flip(0), 0)[-1]]


def loss_in_three_orders(c, name):
    """The loss ``name`` of the tensors ``c`` with its sums taken in the three orders of ``scalar_sums``, as floats."""
    if name == "enhanced":
        terms, w, _ = enhanced_parts(c)
        return [float(a / b) for a, b in zip(scalar_sums(terms), scalar_sums(w))]
    terms, inside = plain_parts(c) if name == "plain" else hole_parts(c)
    count = int(inside.sum()) * (3 if name == "plain" else 1)
    return [float(a / count) for a in scalar_sums(terms)]


def normalised_error(g, g64):
    """max |g - g64| / max |g64|"""
    g64 = np.asarray(g64, dtype=np.float64)
    return float(np.abs(np.asarray(g, dtype=np.float64) - g64).max() / np.abs(g64).max())
