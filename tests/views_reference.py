"""The statements of include/gd_views.h in numpy and torch, and a test PNG encoder that applies a chosen filter type per
row (export.save_image_rgba writes type 0 only).  No test in here: tests/test_views_cpu.py and tests/test_views_gpu.py
import it."""
import struct
import zlib

import numpy as np
import torch

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _paeth(a, b, c):
    """the Paeth predictor of int arrays: ties go to a, then b, then c"""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _predict(kind, a, b, c):
    if kind == 1:
        return a
    if kind == 2:
        return b
    if kind == 3:
        return (a + b) >> 1
    if kind == 4:
        return _paeth(a, b, c)
    return np.zeros_like(a)


def filter_rows(pixels: np.ndarray, kinds) -> np.ndarray:
    """uint8 [H, 1 + W bpp]: ``pixels`` uint8 [H,W,bpp] filtered with type ``kinds[r]`` on row r.  filt = raw - pred(raw):
    the neighbours of the encoder are raw pixels, so every row is one vector expression."""
    H, W, bpp = pixels.shape
    raw = pixels.reshape(H, W * bpp).astype(np.int64)
    left = np.concatenate((np.zeros((H, bpp), np.int64), raw[:, :-bpp]), axis=1)
    up = np.concatenate((np.zeros((1, W * bpp), np.int64), raw[:-1]), axis=0)
    upleft = np.concatenate((np.zeros((H, bpp), np.int64), up[:, :-bpp]), axis=1)
    out = np.zeros((H, 1 + W * bpp), np.uint8)
    for r in range(H):
        kind = int(kinds[r])
        out[r, 0] = kind
        out[r, 1:] = (raw[r] - _predict(kind, left[r], up[r], upleft[r])) & 255
    return out


def chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def encode_png(pixels: np.ndarray, kinds, depth: int = 8, rows: np.ndarray = None) -> bytes:
    """The bytes of a PNG file of ``pixels`` uint8 [H,W,3|4] with row filter ``kinds[r]`` on row r.  ``depth`` goes into the
    header as it is; ``rows`` replaces the filtered rows (for streams no encoder would write)."""
    H, W, bpp = pixels.shape
    rows = filter_rows(pixels, kinds) if rows is None else rows
    header = struct.pack(">IIBBBBB", W, H, depth, 2 if bpp == 3 else 6, 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", header) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b"")


def write_png(path, pixels: np.ndarray, kinds, **kw) -> str:
    with open(path, "wb") as f:
        f.write(encode_png(pixels, kinds, **kw))
    return str(path)


def unfilter(rows: np.ndarray, bpp: int) -> np.ndarray:
    """uint8 [H, W bpp]: the PNG specification's reconstruction of ``rows`` uint8 [H, 1 + W bpp], byte by byte along a row
    (all channels of a pixel at once), a type above 4 as type 0."""
    H, stride = rows.shape[0], rows.shape[1] - 1
    out = np.zeros((H, stride), np.int64)
    zero = np.zeros(bpp, np.int64)
    for r in range(H):
        kind = int(rows[r, 0])
        filt = rows[r, 1:].astype(np.int64)
        prior = out[r - 1] if r else np.zeros(stride, np.int64)
        for i in range(0, stride, bpp):
            a = out[r, i - bpp:i] if i else zero
            c = prior[i - bpp:i] if i else zero
            out[r, i:i + bpp] = (filt[i:i + bpp] + _predict(kind, a, prior[i:i + bpp], c)) & 255
    return out.astype(np.uint8)


def kinds_for(H: int, mode, seed: int = 0) -> np.ndarray:
    """``mode`` 0..4: every row of that type; "mixed": a seeded random type per row"""
    if mode == "mixed":
        return np.random.default_rng(seed).integers(0, 5, size=H)
    return np.full(H, int(mode))


def random_pixels(H, W, bpp, seed) -> np.ndarray:
    """seeded random bytes: Paeth ties and wrap-around everywhere"""
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, bpp), dtype=np.uint8)


def ramp_pixels(H, W, bpp) -> np.ndarray:
    """a smooth ramp: small residuals, long runs of equal predictors"""
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(bpp), indexing="ij")
    return ((3 * x + 2 * y + 40 * c) % 256).astype(np.uint8)


def unpack(normal_rgba: np.ndarray, rgb: np.ndarray):
    """(normal [H,W,3], mask [H,W,1], rgb [H,W,3]) float32 in numpy: every operation one fp32 rounding, in the header's order"""
    one, two = np.float32(1), np.float32(2)
    x = normal_rgba.astype(np.float32) / np.float32(255.0)
    n = x[..., :3] * two - one
    n[..., 1] = n[..., 1] * np.float32(-1)
    return (n + one) / two, x[..., 3:4].copy(), (rgb[..., :3].astype(np.float32) / np.float32(255.0))


def unpack_torch(normal_rgba: np.ndarray, rgb: np.ndarray):
    """the same as ``View.load`` writes it, on CPU tensors"""
    img = torch.FloatTensor((normal_rgba.astype(np.float32) / 255.0).copy())
    mask = img[:, :, -1:]
    normal = img[:, :, :3]
    normal = normal * 2 - 1
    normal[:, :, 1] *= -1
    normal = (normal + 1) / 2
    colour = torch.FloatTensor((rgb.astype(np.float32) / 255.0).copy())[:, :, :3]
    return normal, mask.clone(), colour.clone()


def every_byte_image(seed: int) -> np.ndarray:
    """uint8 [16,16,4] holding every byte value in every channel, each channel in its own seeded order"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256).astype(np.uint8).reshape(16, 16) for _ in range(4)], axis=-1)


def rigid_c2w(seed: int, axis_aligned: bool = False) -> np.ndarray:
    """float32 [4,4]: a seeded rotation (proper, by QR) and position; ``axis_aligned`` looks down -z from (0, 0, 2.5)"""
    c2w = np.eye(4)
    if axis_aligned:
        c2w[:3, 3] = (0.0, 0.0, 2.5)
    else:
        rng = np.random.default_rng(seed)
        q, r = np.linalg.qr(rng.normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        c2w[:3, :3] = q
        c2w[:3, 3] = rng.normal(size=3) * 0.7 + q[:, 2] * 2.5
    return c2w.astype(np.float32)
