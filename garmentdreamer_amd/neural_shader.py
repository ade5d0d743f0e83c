"""The neural shader of the mesh deformer's second stage (the reference's ``deformer/modules/neuralshader.py`` with the
configuration ``deformation.py`` gives it) on the HIP kernels of ``csrc/raster_shader.hip`` and
``csrc/raster_shader_mfma.hip`` (definitions, rounding points, layouts and C-ABI: include/gd_shader.h) -- no CPU path.

``NeuralShader`` holds the sixteen fp32 master tensors under the reference's names as views of ONE flat buffer, their
gradients as views of ONE flat gradient buffer into which the weight-gradient kernels add (the arrangement of
``TextureField`` / ``flat_adam.reseat``), and the two packed bf16 images the products read.  ``shader(position, normal,
view_dir)`` is the no-grad colour of given points (what the reference's preview image calls); the training path is
``mesh_losses.shading_loss``.  ``optimizer()`` is Adam as one ``gd_scene_adam_step`` launch followed by the pack launch.
Whoever writes the parameters by another way calls ``pack()`` afterwards.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, List

import torch

from . import _native
from ._launch import launch, require_gpu, scratch
from .flat_adam import reseat

LAYERS = _native.SHADER_LAYERS
IN_FEATURES = (27, 256, 256, 256, 256, 262, 128, 128)
OUT_FEATURES = (256, 256, 256, 256, 256, 128, 128, 3)
PADDED_IN = (32, 256, 256, 256, 256, 288, 128, 128)
PADDED_OUT = (256, 256, 256, 256, 256, 128, 128, 32)
LAYER_NAMES = [f"diffuse.network.{i}.linear" for i in range(5)] + [f"specular.network.{i}.linear" for i in range(3)]
PARAM_NAMES = [f"{n}.{k}" for n in LAYER_NAMES for k in ("weight", "bias")]
CONFIG = {"hidden_features_size": 256, "hidden_features_layers": 3, "activation": "relu", "fourier_features": "positional",
          "mapping_size": 256, "fft_scale": 4}          # plus "last_activation": a torch.nn.Sigmoid
ACT_WIDTH, DZ_WIDTH = sum(PADDED_IN), sum(PADDED_OUT)   # halves per point of the stored activations and of the dZ


def rows_of(capacity: int) -> int:
    """``gd_shader_rows``: the rows of every per-point buffer"""
    tile = _native.SHADER_TILE_ROWS
    return (int(capacity) + tile - 1) // tile * tile


def act_offset(l: int, rows: int) -> int:
    return rows * sum(PADDED_IN[:l])


def dz_offset(l: int, rows: int) -> int:
    return rows * sum(PADDED_OUT[:l])


def check_capacity(name: str, capacity: int) -> int:
    capacity = int(capacity)
    if not 1 <= capacity <= 1 << 24:
        raise ValueError(f"{name}: capacity must be in [1, 2^24]")
    return capacity


def _check_config(config: Dict) -> None:
    given = dict(config)
    last = given.pop("last_activation", None)
    given.pop("device", None)
    if not isinstance(last, torch.nn.Sigmoid) or given != CONFIG:
        raise ValueError("NeuralShader: the kernels are built for hidden_features_size=256, hidden_features_layers=3, "
                         "activation='relu', last_activation=Sigmoid, fourier_features='positional', mapping_size=256, "
                         f"fft_scale=4 only (got {config})")


class NeuralShader:
    def __init__(self, hidden_features_size=256, hidden_features_layers=3, activation="relu", last_activation=None,
                 fourier_features="positional", mapping_size=256, fft_scale=4, device="cuda", seed: int = 0):
        """The reference's constructor arguments (``last_activation=None`` stands for the Sigmoid of ``deformation.py``);
        any value but the fixed configuration raises.  ``kaiming_normal_(fan_in, relu)`` weights from ``seed``, zero biases."""
        if last_activation is None:
            last_activation = torch.nn.Sigmoid()
        self._config = {"hidden_features_size": hidden_features_size, "hidden_features_layers": hidden_features_layers,
                        "activation": activation, "last_activation": last_activation, "fourier_features": fourier_features,
                        "mapping_size": mapping_size, "fft_scale": fft_scale}
        _check_config(self._config)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("NeuralShader: the HIP kernels have no CPU path (device must be a GPU)")
        generator = torch.Generator().manual_seed(int(seed))
        self._params: "OrderedDict[str, torch.nn.Parameter]" = OrderedDict()
        for name, k, o in zip(LAYER_NAMES, IN_FEATURES, OUT_FEATURES):
            w = torch.empty(o, k)
            torch.nn.init.kaiming_normal_(w, mode="fan_in", nonlinearity="relu", generator=generator)
            self._params[name + ".weight"] = torch.nn.Parameter(w.to(dev))
            self._params[name + ".bias"] = torch.nn.Parameter(torch.zeros(o, device=dev))
        self.flat, self.flat_grad, self._exp_avg, self._exp_avg_sq, _ = reseat(list(self._params.values()))
        if self.flat.numel() != _native.SHADER_PARAM_ELEMS:
            raise RuntimeError("NeuralShader: the flat buffer does not have the layout of include/gd_shader.h")
        self.packed = torch.empty(_native.SHADER_PACKED_ELEMS, dtype=torch.bfloat16, device=dev)
        self.packed_t = torch.empty_like(self.packed)
        self.pack()

    @property
    def device(self) -> torch.device:
        return self.flat.device

    def pack(self) -> None:
        """Round the master weights into the packed images the products read: one launch."""
        launch("gd_shader_pack", self.device, self.flat, self.packed, self.packed_t)

    # ---- the surface of the reference's module ------------------------------------------------------------------------
    def parameters(self) -> List[torch.nn.Parameter]:
        return list(self._params.values())

    def named_parameters(self):
        return list(self._params.items())

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((k, v.detach().clone()) for k, v in self._params.items())

    @torch.no_grad()
    def load_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        if set(state) != set(self._params):
            raise KeyError("NeuralShader.load_state_dict: expected exactly the keys " + ", ".join(PARAM_NAMES))
        for k, p in self._params.items():
            t = torch.as_tensor(state[k])
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"NeuralShader.load_state_dict: {k} must be {tuple(p.shape)}")
            p.copy_(t.to(device=p.device, dtype=torch.float32))
        self.pack()

    def save(self, path) -> None:
        """The reference's file: its ``NeuralShader.load`` reads it."""
        torch.save({"version": 2, "config": dict(self._config),
                    "state_dict": OrderedDict((k, v.cpu()) for k, v in self.state_dict().items())}, path)

    @classmethod
    def load(cls, path, device="cuda") -> "NeuralShader":
        data = torch.load(path, map_location="cpu", weights_only=False)
        _check_config(data["config"])
        shader = cls(**{k: v for k, v in data["config"].items() if k != "device"}, device=device)
        shader.load_state_dict(data["state_dict"])
        return shader

    def optimizer(self, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8) -> "NeuralShaderOptimizer":
        return NeuralShaderOptimizer(self, lr, betas, eps)

    # ---- the no-grad call ---------------------------------------------------------------------------------------------
    def forward_layers(self, capacity: int, counters: torch.Tensor, act: torch.Tensor, logits: torch.Tensor) -> None:
        """The eight forward products over the rows below ``counters[0]``: eight launches"""
        for l in range(LAYERS):
            launch("gd_shader_forward_layer", self.device, l, C.c_int64(capacity), counters, self.packed, self.flat, act, logits)

    @torch.no_grad()
    def __call__(self, position: torch.Tensor, normal: torch.Tensor, view_dir: torch.Tensor) -> torch.Tensor:
        """Colour [..., 3] of the points ``position`` with ``normal`` and ``view_dir``, all float32 [..., 3] on the GPU."""
        name = "NeuralShader"
        given = (("position", position), ("normal", normal), ("view_dir", view_dir))
        if any(not isinstance(t, torch.Tensor) or t.dim() < 2 or t.shape[-1] != 3 or t.shape != position.shape for _, t in given):
            raise ValueError(f"{name}: position, normal and view_dir must be tensors of one shape [..., 3]")
        for what, t in given:
            require_gpu(name, what, t, torch.float32, 3)
        shape, dev = position.shape, self.device
        n = position.numel() // 3
        if n == 0:
            return torch.empty(shape, dtype=torch.float32, device=dev)
        capacity = check_capacity(name, n)
        rows = rows_of(capacity)
        counters = torch.empty(4, dtype=torch.int32, device=dev)
        act = torch.empty(rows * ACT_WIDTH, dtype=torch.bfloat16, device=dev)
        logits = torch.empty(rows, 3, dtype=torch.float32, device=dev)
        launch("gd_shader_features_points", dev, C.c_int64(n), position.detach().reshape(-1, 3).contiguous(),
               normal.detach().reshape(-1, 3).contiguous(), view_dir.detach().reshape(-1, 3).contiguous(),
               C.c_int64(capacity), counters, act)
        self.forward_layers(capacity, counters, act, logits)
        colour = torch.empty(n, 3, dtype=torch.float32, device=dev)
        launch("gd_shader_colour", dev, C.c_int64(n), logits, colour)
        return colour.reshape(shape)

    forward = __call__


class NeuralShaderOptimizer:
    """``torch.optim.Adam(shader.parameters(), lr)`` as ONE ``gd_scene_adam_step`` launch over the flat buffer, followed by the
    pack launch; ``zero_grad`` is ONE memset.  As with ``FlatAdam``, a parameter always has a gradient here."""

    def __init__(self, shader: NeuralShader, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        self.shader = shader
        self.param_groups = [{"params": shader.parameters(), "lr": float(lr)}]
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.step_count = 0
        self._ends = (C.c_int64 * 1)(shader.flat.numel())

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.shader.flat_grad.zero_()

    @torch.no_grad()
    def step(self) -> None:
        s = self.shader
        self.step_count += 1
        lrs = (C.c_double * 1)(float(self.param_groups[0]["lr"]))
        launch("gd_scene_adam_step", s.device, s.flat, s.flat_grad, s._exp_avg, s._exp_avg_sq, s.flat.numel(), 1, self._ends,
               lrs, self.betas[0], self.betas[1], self.eps, self.step_count)
        s.pack()


def workspace(capacity: int, dev) -> torch.Tensor:
    """The scratch of the L1 and of the weight gradients for ``capacity`` points"""
    return scratch(_native.lib().gd_shader_scratch_bytes(capacity), dev)
