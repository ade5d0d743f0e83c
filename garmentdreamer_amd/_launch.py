"""The one way from a torch tensor to an entry of ``libgd_raster.so`` or ``libgd_nn.so``: what every op does around its
kernel, written once."""
from __future__ import annotations

from typing import Optional

import torch

from . import _native


def call(fn, dev, args):
    """``fn`` on ``dev``'s current stream (its first argument) with ``args``, tensors as their ``data_ptr()`` and
    everything else (``None``, numbers, ctypes values) as it is; returns what ``fn`` returns.  Layout is the caller's
    business: nothing here copies, allocates or waits."""
    with torch.cuda.device(dev):
        return fn(torch.cuda.current_stream(dev).cuda_stream,
                  *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])


def launch(name: str, dev, *args) -> int:
    """``call`` of the entry ``name`` of libgd_raster.so; raises with the entry's error text if it fails.
    (``nn_ops.launch`` is the same for libgd_nn.so.)"""
    return _native.checked(name, call(getattr(_native.lib(), name), dev, args))


def scratch(nbytes: int, dev) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def require_gpu(name: str, what: str, t, dtype=None, last: Optional[int] = None) -> torch.Tensor:
    """``t`` if it is a tensor on the GPU, of ``dtype`` if one is given and [..., ``last``] if that is."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name}: the HIP kernels have no CPU path ({what} must be on the GPU)")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: {what} must be {dtype}")
    if last is not None and (t.dim() < 2 or t.shape[-1] != last):
        raise ValueError(f"{name}: {what} must be [..., {last}]")
    return t
