"""On-disk products either side of the path: the per-view RGBA PNG + ``cameras.json`` dump that
stages 3-4 consume (Garment_3DGS/threestudio/systems/GaussianDreamer.py:330-417, utils/saving.py:331-354) and the
prompt-embedding cache key (models/prompt_processors/base.py:19-23).  ``last_3dgs.ply`` lives in
``gaussian_model.GaussianModel.save_ply``.  Pure Python / numpy (the reference uses cv2, absent here)."""
from __future__ import annotations

import hashlib
import json
import math
import os
import struct
import zlib
from typing import Dict, List

import numpy as np


def fov2focal(fov, pixels):
    """gaussiansplatting/utils/graphics_utils.py:95-96"""
    return pixels / (2 * math.tan(fov / 2))


def focal2fov(focal, pixels):
    """gaussiansplatting/utils/graphics_utils.py:98-99"""
    return 2 * math.atan(pixels / (2 * focal))


def hash_prompt(model: str, prompt: str) -> str:
    """Cache key of a prompt's text embeddings: ``<cache_dir>/<md5(model-prompt)>.pt`` (base.py:19-23,413-422)."""
    return hashlib.md5(f"{model}-{prompt}".encode()).hexdigest()


def camera_info_entry(c2w, index: int, width: int, height: int, fovy: float) -> Dict:
    """One ``cameras.json`` record (GaussianDreamer.py:351-362): position = c2w translation, rotation = the
    NEGATED c2w rotation (``rot[:, :] *= -1``), fy from fovy, fx through the fov round trip the reference does."""
    C2W = np.array(c2w, dtype=np.float32, copy=True)
    pos = C2W[:3, 3]
    rot = C2W[:3, :3] * -1
    fy = fov2focal(float(fovy), height)
    return {"id": int(index), "img_name": str(int(index)), "width": width, "height": height,
            "position": pos.tolist(), "rotation": [x.tolist() for x in rot], "fy": fy,
            "fx": fov2focal(focal2fov(fy, width), width)}


def save_cameras_json(path: str, camera_info_list: List[Dict]):
    """GaussianDreamer.py:330-332"""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(camera_info_list, f)


def _png_chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def save_image_rgba(path: str, rgb, mask) -> str:
    """``save_image_rgba`` (saving.py:331-354): rgb [H,W,3] in [0,1], mask [H,W] in {0,1} -> 8-bit RGBA PNG
    (clip, x255, round to nearest even like cv2's saturate_cast).  ``rgb`` / ``mask``: numpy or torch."""
    to_np = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)   # noqa: E731
    rgb, mask = to_np(rgb).astype(np.float32), to_np(mask).astype(np.float32)
    assert mask.max() <= 1.0
    img = np.concatenate((rgb, mask[..., None]), axis=-1).clip(0, 1) * np.float32(255.0)
    img8 = np.rint(img).astype(np.uint8)
    H, W = img8.shape[:2]
    raw = np.concatenate((np.zeros((H, 1), np.uint8), img8.reshape(H, W * 4)), axis=1).tobytes()   # filter 0 per row
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(_png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0)))   # 8-bit, colour type 6 = RGBA
        f.write(_png_chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(_png_chunk(b"IEND", b""))
    return path


def save_image_rgb(path: str, rgb8) -> str:
    """uint8 [H,W,3] (numpy or torch) -> 8-bit RGB PNG, bytes as given, row 0 first (the baked albedo of
    ``texture_bake.write_textured_obj``)."""
    img8 = rgb8.detach().cpu().numpy() if hasattr(rgb8, "detach") else np.asarray(rgb8)
    if img8.dtype != np.uint8 or img8.ndim != 3 or img8.shape[2] != 3:
        raise ValueError("save_image_rgb: the image must be uint8 [H,W,3]")
    H, W = img8.shape[:2]
    raw = np.concatenate((np.zeros((H, 1), np.uint8), img8.reshape(H, W * 3)), axis=1).tobytes()   # filter 0 per row
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(_png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)))   # 8-bit, colour type 2 = RGB
        f.write(_png_chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(_png_chunk(b"IEND", b""))
    return path


def read_png_stream(path: str):
    """``(W, H, bpp, rows)`` of the PNG ``load_image_rgb`` reads: the chunks parsed and their CRCs checked, the header
    checked, the IDAT data inflated (``zlib`` releases the GIL) and its length checked.  ``rows``: the ``H (1 + W bpp)``
    bytes of the filtered rows, each with its filter type first; the types themselves are the caller's to check.  The one
    parser of ``load_image_rgb`` and of ``views.decode_png_batch``."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG file (signature)")
    at, header, idat, ended = 8, None, [], False
    while at + 8 <= len(data) and not ended:
        (length,), tag = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + length]
        if len(body) != length or at + 12 + length > len(data):
            raise ValueError(f"{path}: truncated {tag!r} chunk")
        if struct.unpack(">I", data[at + 8 + length:at + 12 + length])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError(f"{path}: CRC mismatch in the {tag!r} chunk")
        if tag == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            ended = True
        at += 12 + length
    if header is None or not idat or not ended:
        raise ValueError(f"{path}: missing IHDR, IDAT or IEND chunk")
    W, H, depth, colour, compression, filtering, interlace = header
    if depth != 8:
        raise ValueError(f"{path}: bit depth {depth} is not supported (8 only)")
    if colour not in (2, 6):
        raise ValueError(f"{path}: colour type {colour} is not supported (2 = RGB and 6 = RGBA only)")
    if interlace != 0:
        raise ValueError(f"{path}: interlaced (Adam7) images are not supported")
    if compression != 0 or filtering != 0 or W < 1 or H < 1:
        raise ValueError(f"{path}: unknown compression or filter method, or an empty image")
    bpp = 3 if colour == 2 else 4
    stride = W * bpp
    raw = zlib.decompress(b"".join(idat))
    if len(raw) != H * (stride + 1):
        raise ValueError(f"{path}: {len(raw)} bytes of pixel data, expected {H * (stride + 1)}")
    return W, H, bpp, raw


def undefined_row_filter(path: str, kind: int) -> ValueError:
    return ValueError(f"{path}: row filter type {kind} is not defined")


def load_image_rgb(path: str) -> np.ndarray:
    """uint8 [H,W,3] or [H,W,4] of an 8-bit PNG of colour type 2 (RGB) or 6 (RGBA), not interlaced, row filters 0-4: what
    ``save_image_rgb`` / ``save_image_rgba`` write and what other writers make of the same pixels.  Anything else (another
    bit depth or colour type, interlacing, a broken file) raises ``ValueError`` naming it.  ``zlib`` and ``struct`` only."""
    W, H, bpp, raw = read_png_stream(path)
    stride = W * bpp
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, stride + 1)
    out = np.zeros((H, stride), dtype=np.uint8)
    prior = np.zeros(stride, dtype=np.int64)
    for r in range(H):
        kind, line = int(rows[r, 0]), rows[r, 1:].astype(np.int64)
        if kind == 0:
            cur = line
        elif kind == 2:                                            # Up
            cur = (line + prior) & 255
        elif kind == 1:                                            # Sub: a running sum per channel
            cur = (np.cumsum(line.reshape(W, bpp), axis=0) & 255).reshape(stride)
        elif kind in (3, 4):                                       # Average, Paeth: each byte needs its left neighbour
            cur = np.zeros(stride, dtype=np.int64)
            src, up = line.tolist(), prior.tolist()
            res = [0] * stride
            for i in range(stride):
                a = res[i - bpp] if i >= bpp else 0
                b = up[i]
                if kind == 3:
                    pred = (a + b) >> 1
                else:
                    c = up[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                res[i] = (src[i] + pred) & 255
            cur[:] = res
        else:
            raise undefined_row_filter(path, kind)
        out[r] = cur
        prior = cur
    return out.reshape(H, W, bpp)


def dump_test_view(save_dir: str, out: Dict, batch: Dict, camera_info_list: List[Dict], alpha_threshold: float = 0.5,
                   view: int = 0):
    """``test_step`` (GaussianDreamer.py:334-410) for one rendered view: thresholded alpha as the mask, RGBA PNG
    under ``gs_rendered_rgba/<index>.png``, one record appended to ``camera_info_list``."""
    alpha = out["alphas"][view].squeeze()
    rgb = out["comp_rgb"][view].squeeze()
    mask = (alpha >= alpha_threshold).to(rgb.dtype) if hasattr(alpha, "to") else (alpha >= alpha_threshold).astype(np.float32)
    idx = int(batch["index"][view])
    fovy = float(batch["fovy"][view])
    c2w = batch["c2w"][view]
    c2w = c2w.detach().cpu().numpy() if hasattr(c2w, "detach") else c2w
    camera_info_list.append(camera_info_entry(c2w, idx, batch["width"], batch["height"], fovy))
    return save_image_rgba(os.path.join(save_dir, "gs_rendered_rgba", f"{idx}.png"), rgb, mask)
