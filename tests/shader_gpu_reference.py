"""What tests/test_shader_gpu.py needs around tests/shader_reference.py: the buffers of include/gd_shader.h as torch tensors
with accessors by layer, calls of the product entries, the rounded statement with its sums taken in a given order, and the
float32 / float64 statements of the element-wise kernels (features, L1, feature backward)."""
import ctypes as C

import numpy as np
import torch

from tests import shader_reference as sref

DEV = "cuda:0"
KP = (32, 256, 256, 256, 256, 288, 128, 128)
OP = (256, 256, 256, 256, 256, 128, 128, 32)
K, O = sref.IN_FEATURES, sref.OUT_FEATURES


def lib():
    from garmentdreamer_amd import _native
    return _native.lib()


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def call(name, *args):
    """An entry on the current stream, tensors as pointers; asserts success with the entry's own message."""
    L = lib()
    ret = getattr(L, name)(stream(), *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])
    assert ret == 0, (name, ret, L.gd_mesh_last_error())


def rows_of(capacity):
    return (capacity + 127) // 128 * 128


def flat_params(ws, bs):
    """float32 [PARAM_ELEMS] on the GPU in the header's layout from eight weights and eight biases (arrays)"""
    from garmentdreamer_amd import _native
    flat = np.zeros(_native.SHADER_PARAM_ELEMS, dtype=np.float32)
    off = 0
    for w, b in zip(ws, bs):
        for a in (w, b):
            a = np.asarray(a, dtype=np.float32).reshape(-1)
            flat[off:off + a.size] = a
            off += (a.size + 63) // 64 * 64
    assert off == flat.size
    return torch.from_numpy(flat).to(DEV)


def param_slices():
    """[(weight offset, bias offset)] per layer in the flat buffers"""
    out, off = [], 0
    for k, o in zip(K, O):
        out.append((off, off + (o * k + 63) // 64 * 64))
        off = out[-1][1] + (o + 63) // 64 * 64
    return out


class Buffers:
    """The per-point buffers for ``n`` points at ``capacity`` (n by default), zero-filled, with ``count = n`` on the device."""

    def __init__(self, n, params, capacity=None, grad_fill=0.0):
        from garmentdreamer_amd import _native
        self.n, self.capacity = n, capacity or max(n, 1)
        self.rows = rows = rows_of(self.capacity)
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=DEV)
        self.act = z(rows * sum(KP), dtype=torch.bfloat16)
        self.dz = z(rows * sum(OP), dtype=torch.bfloat16)
        self.logits, self.dfeat, self.dextra = z(rows, 3), z(rows, 32), z(rows, 32)
        self.counters = torch.tensor([n, 0, n, 0], dtype=torch.int32, device=DEV)
        self.params = params
        self.grad = torch.full_like(params, grad_fill)
        self.packed = z(_native.SHADER_PACKED_ELEMS, dtype=torch.bfloat16)
        self.packed_t = torch.zeros_like(self.packed)
        self.scratch = torch.empty(max(lib().gd_shader_scratch_bytes(self.capacity), 1), dtype=torch.uint8, device=DEV)
        call("gd_shader_pack", params, self.packed, self.packed_t)

    def X(self, l):
        off = self.rows * sum(KP[:l])
        return self.act[off:off + self.rows * KP[l]].view(self.rows, KP[l])

    def dZ(self, l):
        off = self.rows * sum(OP[:l])
        return self.dz[off:off + self.rows * OP[l]].view(self.rows, OP[l])

    def W(self, l, transposed=False):
        off = sref.packed_offset(l)
        src = self.packed_t if transposed else self.packed
        shape = (KP[l], OP[l]) if transposed else (OP[l], KP[l])
        return src[off:off + KP[l] * OP[l]].view(*shape)

    def dW(self, l):
        w, b = param_slices()[l]
        return self.grad[w:w + O[l] * K[l]].view(O[l], K[l]), self.grad[b:b + O[l]]

    def forward(self, l):
        call("gd_shader_forward_layer", l, C.c_int64(self.capacity), self.counters, self.packed, self.params, self.act, self.logits)

    def backward_input(self, l):
        call("gd_shader_backward_input_layer", l, C.c_int64(self.capacity), self.counters, self.packed_t, self.act, self.dz,
             self.dfeat, self.dextra)

    def backward_weight(self, l):
        call("gd_shader_backward_weight_layer", l, C.c_int64(self.capacity), self.counters, self.act, self.dz, self.grad,
             self.scratch)


def to_bf16(a):
    """a float array (values bf16 holds exactly, or to be rounded) as a bf16 GPU tensor"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(torch.bfloat16)


def f64(t):
    return t.detach().to(torch.float64).cpu()


# ---- the rounded statement with its sums in a given order -----------------------------------------------------------------

ORDERS = (None, (32, False), (32, True), (64, False), (64, True))     # plain; chunk width, descending


def product(a, b, order):
    """a @ b with the summed index taken in chunks of ``order[0]``, ascending or descending, each chunk by torch's matmul and
    the chunks added one after the other in the dtype of ``a``"""
    if order is None:
        return a @ b
    width, descending = order
    starts = list(range(0, a.shape[1], width))
    if descending:
        starts.reverse()
    total = None
    for s in starts:
        part = a[:, s:s + width] @ b[s:s + width]
        total = part if total is None else total + part
    return total


def rounded_ordered(case, params, dtype, keep, order):
    """``sref.rounded`` with every product through ``product(..., order)``: dict with loss, dposition, dnormal, dW, db"""
    with torch.no_grad():
        position, normal, center, rgb = (t.detach() for t in sref._inputs(case, dtype))
        ws, bs = (list(t.detach() for t in ts) for ts in sref.param_tensors(params, dtype))
        k = torch.from_numpy(keep)
        count = int(keep.sum())
        p, n, target = position[k], normal[k], rgb[k]
        v = center - p
        length = v.norm(dim=-1, keepdim=True)
        u = v / length.clamp_min(sref.NORM_EPS)
        wq = [sref.bf16(w) for w in ws]
        X = [sref.bf16(sref.encode(p))]
        for l in range(8):
            if l == 5:
                X[5] = torch.cat([X[5], sref.bf16(torch.cat([n, u], dim=-1))], dim=-1)
            z = product(X[l], wq[l].T, order) + bs[l]
            if l == 7:
                logits = z
            else:
                X.append(sref.bf16(torch.relu(z) if sref.RELU[l] else z))
        c = torch.sigmoid(logits)
        loss = (c - target).abs().sum() / (3 * count)
        dZ = [None] * 8
        dZ[7] = sref.bf16(torch.sign(c - target) * (c * (1 - c)) / (3 * count))
        dW, db = [None] * 8, [None] * 8
        for l in range(7, -1, -1):
            dW[l] = product(dZ[l].T, X[l], order)
            db[l] = product(dZ[l].T, torch.ones(dZ[l].shape[0], 1, dtype=dtype), order)[:, 0]
            dX = product(dZ[l], wq[l], order)
            if l == 0:
                dfeat = dX
            elif l == 5:
                dextra = dX[:, 256:]
                dZ[4] = sref.bf16(dX[:, :256])
            else:
                dZ[l - 1] = sref.bf16(torch.where(X[l] > 0, dX, torch.zeros_like(dX)))
        dp, dn = features_backward(p, center, dfeat, dextra)
        dposition, dnormal = torch.zeros_like(position), torch.zeros_like(normal)
        dposition[k], dnormal[k] = dp, dn
        shape = case["position"].shape
        return {"loss": float(loss), "dposition": dposition.numpy().reshape(shape), "dnormal": dnormal.numpy().reshape(shape),
                "dW": [w.numpy() for w in dW], "db": [b.numpy() for b in db]}


# ---- the element-wise kernels, by dtype ----------------------------------------------------------------------------------

def features(p, n, center):
    """(feat [N,27], extra [N,6]) unrounded in the dtype of ``p``"""
    return sref.encode(p), torch.cat([n, sref.view_dir(p, center)], dim=-1)


def l1(logits, target, dloss=1.0):
    """(the terms |c - t| [N,3], dlogits, c) of include/gd_shader.h LOSS in the dtype of ``logits``"""
    count = logits.shape[0]
    c = 1 / (1 + torch.exp(-logits))
    return (c - target).abs(), torch.sign(c - target) * ((dloss / (3 * count)) * (c * (1 - c))), c


def features_backward(p, center, dfeat, dextra):
    """(dposition, dnormal) [N,3] of include/gd_shader.h FEATURES backward in the dtype of ``p``"""
    dp = dfeat[:, :3].clone()
    for j, f in enumerate(sref.FREQUENCIES):
        dp = dp + f * (torch.cos(f * p) * dfeat[:, 3 + 6 * j:6 + 6 * j] - torch.sin(f * p) * dfeat[:, 6 + 6 * j:9 + 6 * j])
    v = center - p
    length = v.norm(dim=-1, keepdim=True)
    u = v / length.clamp_min(sref.NORM_EPS)
    gu = dextra[:, 3:6]
    gv = torch.where(length > sref.NORM_EPS, (gu - u * (u * gu).sum(-1, keepdim=True)) / length.clamp_min(sref.NORM_EPS),
                     gu / sref.NORM_EPS)
    return dp - gv, dextra[:, :3]


def relative_l2(a, b):
    """|a - b| / |b| over all entries"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
