"""The statement of the deformer's neural shader and shading loss (tests/shader_reference.py; the definition:
include/gd_shader.h), pinned before any kernel exists: the header's C (``hash32``, the threshold, the layer and packing
tables) against the Python restatement bit for bit, both dtypes against values the reference's own code produced
(tests/golden/shader_pins.npz), float64 autograd against central differences, its two forms against each other, the Python
``hash32`` subset, and the exact-integer cases a kernel test is to run against the magnitude at which bf16 still holds every
integer.  No kernel and nothing of the package is run here."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import mesh_losses_reference as lref
from tests import shader_reference as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT_SIZES = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300)


def _pins():
    return np.load(os.path.join(ROOT, "tests", "golden", "shader_pins.npz"))


def _pinned_case(pins, name):
    return {k: pins[f"{name}/{k}"] for k in sref.GOLDEN_INPUT_KEYS}


# ---- the header ------------------------------------------------------------------------------------------------------------

HEADER_PROBE = """
#include "gd_shader.h"
uint32_t probe_hash32(uint32_t seed, uint32_t step, uint32_t pixel) { return gd_shader_hash32(seed, step, pixel); }
uint32_t probe_threshold(float p) { return gd_shader_keep_threshold(p); }
int probe_in(int l, int padded) { return gd_shader_in(l, padded); }
int probe_out(int l, int padded) { return gd_shader_out(l, padded); }
int probe_relu(int l) { return gd_shader_relu(l); }
size_t probe_offset(int l) { return gd_shader_packed_offset(l); }
int probe_layers(void) { return GD_SHADER_LAYERS; }
size_t probe_packed(void) { return GD_SHADER_PACKED_ELEMS; }
"""


def test_the_headers_c_is_the_python_statement_bit_for_bit(tmp_path):
    """include/gd_shader.h compiled as C on the host (what this test is about: the one process it starts is the compiler)."""
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a host C compiler (the one that builds oracle/) is needed"
    src, lib = tmp_path / "probe.c", tmp_path / "probe.so"
    src.write_text(HEADER_PROBE)
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           "-o", str(lib), str(src)])
    L = ctypes.CDLL(str(lib))
    L.probe_hash32.restype = L.probe_threshold.restype = ctypes.c_uint32
    L.probe_hash32.argtypes = [ctypes.c_uint32] * 3
    L.probe_threshold.argtypes = [ctypes.c_float]
    L.probe_offset.restype = L.probe_packed.restype = ctypes.c_size_t
    rng = np.random.RandomState(1)
    triples = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (2 ** 32 - 1,) * 3] + \
        [tuple(int(v) for v in rng.randint(0, 2 ** 32, 3, dtype=np.uint64)) for _ in range(2000)]
    for seed, step, pixel in triples:
        assert L.probe_hash32(seed, step, pixel) == int(sref.hash32(seed, step, pixel)), (seed, step, pixel)
    for p in (0.0, 0.25, 0.75, 0.1, 1e-10, float(np.nextafter(np.float32(1), np.float32(0)))):
        assert L.probe_threshold(p) == int(sref.keep_threshold(p)), p
    assert L.probe_layers() == 8 == len(sref.NAMES)
    for l in range(8):
        assert (L.probe_in(l, 0), L.probe_out(l, 0), bool(L.probe_relu(l))) == (sref.IN_FEATURES[l], sref.OUT_FEATURES[l], sref.RELU[l])
        assert L.probe_in(l, 1) % 32 == 0 and L.probe_out(l, 1) % 32 == 0
        assert 0 <= L.probe_in(l, 1) - L.probe_in(l, 0) < 32 and 0 <= L.probe_out(l, 1) - L.probe_out(l, 0) < 32
        assert L.probe_offset(l) == sref.packed_offset(l)
    assert L.probe_offset(8) == L.probe_packed() == sref.packed_offset(8) == 327680


# ---- the reference, pinned ------------------------------------------------------------------------------------------------

# Sixteen products in a chain (eight forward, eight backward), each a float32 sum of up to 262 terms whose order differs from
# the reference's BLAS.  Rounding errors of a sum of K terms add like a random walk, sqrt(K) 2^-24 = 9.6e-7 for K = 262; the
# sixteen are taken to add in full: 16 sqrt(262) 2^-24 = 1.5e-5 of the largest entry.  The pins carry the same error, so the
# float64 statement is held to the same bound.
PIN_BOUND = 16 * np.sqrt(262.0) * 2.0 ** -24


@pytest.mark.parametrize("gather", (True, False), ids=("gather", "masked"))
def test_both_dtypes_agree_with_the_golden_pins(gather):
    pins = _pins()
    params = sref.make_params(int(pins["seed"]))
    means = {torch.float32: 0.0, torch.float64: 0.0}
    for name in sref.GOLDEN_CASES:
        case = _pinned_case(pins, name)
        assert all(np.array_equal(case[k], v) for k, v in sref.golden_cases()[name].items() if k in case)
        for dtype in (torch.float32, torch.float64):
            keep = sref.valid_pixels(case, dtype)
            assert 10 < keep.sum() < keep.shape[0]
            got = sref.unrounded(case, params, dtype, keep, gather)
            means[dtype] += got["loss"] / len(sref.GOLDEN_CASES)
            worst = abs(got["loss"] - float(pins[f"{name}/loss"])) / float(pins[f"{name}/loss"])
            for k in ("dposition", "dnormal"):
                want = pins[f"{name}/{k}"]
                assert np.abs(want).max() > 0 and not want.reshape(-1, 3)[~keep].any()
                worst = max(worst, sref.normalised_error(got[k], want))
            for l, layer in enumerate(sref.NAMES):
                worst = max(worst, sref.normalised_error(got["db"][l], pins[f"{name}/{layer}.bias"]))
                dw = got["dW"][l].astype(np.float64)
                rows, sums = pins[f"{name}/{layer}.weight/rows"], pins[f"{name}/{layer}.weight/sums"]
                worst = max(worst, np.abs(dw[[0, 1, -1]] - rows).max() / np.abs(dw).max())
                worst = max(worst, abs(dw.sum() - sums[0]) / np.sqrt(dw.size * sums[1]), abs((dw ** 2).sum() - sums[1]) / (2 * sums[1]))
            print(f"{name} {'gather' if gather else 'masked'} {dtype}: largest normalised difference to the pins {worst:.3e}")
            assert worst <= PIN_BOUND, (name, dtype)
    for dtype, mean in means.items():
        assert abs(mean - float(pins["both/loss"])) <= PIN_BOUND * mean


def test_the_masked_sum_and_the_gather_form_agree():
    """float64: the two forms differ by the order of sums and by F.normalize against the written division."""
    pins = _pins()
    params = sref.make_params(int(pins["seed"]))
    case = _pinned_case(pins, "view0")
    keep = sref.valid_pixels(case, torch.float64)
    a, b = (sref.unrounded(case, params, torch.float64, keep, g) for g in (True, False))
    assert abs(a["loss"] - b["loss"]) <= 1e-13 * a["loss"]
    for k in ("dposition", "dnormal", "colour"):
        assert sref.normalised_error(a[k], b[k]) <= 1e-12, k
    for k in ("dW", "db"):
        assert all(sref.normalised_error(x, y) <= 1e-12 for x, y in zip(a[k], b[k])), k
    none = np.zeros_like(keep)
    for g in (True, False):
        empty = sref.unrounded(case, params, torch.float64, none, g)
        assert empty["loss"] == 0 and not empty["dposition"].any() and not any(w.any() for w in empty["dW"])
    assert sref.rounded(case, params, torch.float32, none)["loss"] == 0


def test_float64_autograd_against_central_differences():
    """Steps of 1e-6 in quantities of order 1: truncation ~1e-12, rounding ~1e-16 / 1e-6, against gradients of ~1e-3: asserted
    at 1e-5 of the largest gradient entry.  (A ReLU whose argument lies within the step of 0 would show as an error of the
    order of one unit's share; none of the probed entries has one.)"""
    pins = _pins()
    params = sref.make_params(int(pins["seed"]))
    case = _pinned_case(pins, "view0")
    keep = sref.valid_pixels(case, torch.float64)
    base = sref.unrounded(case, params, torch.float64, keep)
    rng = np.random.RandomState(0)
    pixels = rng.choice(np.flatnonzero(keep), 4, replace=False)
    h = 1e-6
    for key in ("position", "normal"):
        grad = base["d" + key].reshape(-1, 3)
        for i in pixels:
            for c in range(3):
                losses = []
                for s in (+1, -1):
                    moved = dict(case)
                    a = case[key].astype(np.float64).reshape(-1, 3).copy()
                    a[i, c] += s * h
                    moved[key] = a.reshape(case[key].shape)
                    losses.append(sref.unrounded(moved, params, torch.float64, keep)["loss"])
                numeric = (losses[0] - losses[1]) / (2 * h)
                assert abs(numeric - grad[i, c]) <= 1e-5 * np.abs(grad).max(), (key, i, c, numeric, grad[i, c])


def test_the_hashed_subset():
    case = lref.make_case(64, 64, 13)
    valid = sref.valid_pixels(case, torch.float64)
    n, p = int(valid.sum()), 0.75
    a = sref.kept_pixels(case, torch.float64, p, seed=5, step=0)
    assert np.array_equal(a, sref.kept_pixels(case, torch.float64, p, seed=5, step=0))
    assert not (a & ~valid).any() and np.array_equal(sref.kept_pixels(case, torch.float64, 1.0), valid)
    b = sref.kept_pixels(case, torch.float64, p, seed=5, step=1)
    assert not np.array_equal(a, b) and not np.array_equal(a, sref.kept_pixels(case, torch.float64, p, seed=6, step=0))
    for kept in (a, b):
        assert abs(int(kept.sum()) - n * p) <= 6 * np.sqrt(n * p * (1 - p)), (int(kept.sum()), n)
    assert not sref.kept_pixels(case, torch.float64, 0.0).any()
    assert [int(v) for v in sref.hash32(0, 0, [0, 1])] == [int(sref.hash32(0, 0, 0)), int(sref.hash32(0, 0, 1))]
    assert int(sref.hash32(0, 0, 0)) == 0 and int(sref.hash32(0, 0, 1)) != int(sref.hash32(0, 1, 1)) != int(sref.hash32(1, 0, 1))


@pytest.mark.parametrize("dense", range(8))
def test_the_exact_integer_cases_stay_where_bf16_holds_every_integer(dense):
    """Every activation, every dX and every logit of the exact-integer cases is an integer of magnitude <= 256
    (bf16 has eight significant bits), the weight gradients stay below 2^24, and more than a third of the dense layer's
    forward products are nonzero."""
    for n in EXACT_SIZES:
        case = sref.exact_case(dense, n, 1000 * dense + n)
        logits, dfeat, dextra, dW, db, X, dZ = sref.exact_expected(case)
        for t in [logits, dfeat, dextra] + X + dZ:
            assert float(t.abs().max()) <= 256 and torch.equal(t, t.round())
            assert torch.equal(sref.bf16(t), t)
        assert all(float(t.abs().max()) < 2 ** 24 for t in dW + db)
        w = torch.from_numpy(case["ws"][dense])
        nonzero = ((X[dense] != 0).double() @ (w != 0).double().T).sum() / (n * w.numel())
        assert float(nonzero) > 1 / 3, (dense, n, float(nonzero))
        if n == 300:                               # and no result is trivially zero
            assert all(t.abs().max() > 0 for t in [logits, dfeat, dextra[:, :3], dextra[:, 3:]] + dW + db)
